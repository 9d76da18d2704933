// oracle/ref_shim/cuda_runtime.h  --  TEST INFRASTRUCTURE.
//
// Stand-in for the CUDA headers that the reference's device code includes, so that a host C++ compiler reads
// that code as plain C++ (oracle/ref_driver.cpp, the `_ref/libegr_reference.so` target of oracle/Makefile).
// Written from what the compiler asks for when it meets the reference's sources; no reference text in here.
// The other CUDA header names of this directory forward to this file.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <math.h> // ::exp(float), ::log(float), ::tan(float) ... as overloads, like in device code

// ---- function and variable qualifiers: nothing on the host
#define __device__
#define __host__
#define __global__
#define __constant__
#define __restrict__
#define __forceinline__ inline
#define __inline__ inline

// ---- vector types, 1 to 4 components (plain aggregates: `return {a, b, c};` must work)
#define EGR_SHIM_VEC(T, name)                                                     \
    struct name##1 { T x; };                                                      \
    struct name##2 { T x, y; };                                                   \
    struct name##3 { T x, y, z; };                                                \
    struct name##4 { T x, y, z, w; };                                             \
    inline name##1 make_##name##1(T x) { return {x}; }                            \
    inline name##2 make_##name##2(T x, T y) { return {x, y}; }                    \
    inline name##3 make_##name##3(T x, T y, T z) { return {x, y, z}; }            \
    inline name##4 make_##name##4(T x, T y, T z, T w) { return {x, y, z, w}; }
EGR_SHIM_VEC(char, char)
EGR_SHIM_VEC(unsigned char, uchar)
EGR_SHIM_VEC(short, short)
EGR_SHIM_VEC(unsigned short, ushort)
EGR_SHIM_VEC(int, int)
EGR_SHIM_VEC(unsigned int, uint)
EGR_SHIM_VEC(long long, longlong)
EGR_SHIM_VEC(unsigned long long, ulonglong)
EGR_SHIM_VEC(float, float)
EGR_SHIM_VEC(double, double)
#undef EGR_SHIM_VEC

// ---- kernel launch coordinates: the driver sets them before it calls a __global__ function's body
extern uint3 threadIdx, blockIdx, blockDim;

// ---- bit casts
inline float __uint_as_float(unsigned int u) {
    float f;
    std::memcpy(&f, &u, sizeof f);
    return f;
}
inline unsigned int __float_as_uint(float f) {
    unsigned int u;
    std::memcpy(&u, &f, sizeof u);
    return u;
}

// ---- min / max. On floats CUDA's are IEEE minNum / maxNum (a NaN operand is dropped), i.e. fminf / fmaxf.
inline float min(float a, float b) { return fminf(a, b); }
inline float max(float a, float b) { return fmaxf(a, b); }
inline double min(double a, double b) { return fmin(a, b); }
inline double max(double a, double b) { return fmax(a, b); }
inline int min(int a, int b) { return a < b ? a : b; }
inline int max(int a, int b) { return a > b ? a : b; }
inline unsigned int min(unsigned int a, unsigned int b) { return a < b ? a : b; }
inline unsigned int max(unsigned int a, unsigned int b) { return a > b ? a : b; }
inline long long min(long long a, long long b) { return a < b ? a : b; }
inline long long max(long long a, long long b) { return a > b ? a : b; }
inline unsigned long long min(unsigned long long a, unsigned long long b) { return a < b ? a : b; }
inline unsigned long long max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// ---- atomicAdd: the driver is single-threaded, so a plain add that returns the old value
inline float atomicAdd(float *p, float v) {
    float o = *p;
    *p = o + v;
    return o;
}
inline int atomicAdd(int *p, int v) {
    int o = *p;
    *p = o + v;
    return o;
}
inline unsigned int atomicAdd(unsigned int *p, unsigned int v) {
    unsigned int o = *p;
    *p = o + v;
    return o;
}
// (an int counter bumped by an unsigned count, and the reverse: device code converts, a template would not deduce)
inline int atomicAdd(int *p, unsigned int v) { return atomicAdd(p, (int)v); }
inline unsigned int atomicAdd(unsigned int *p, int v) { return atomicAdd(p, (unsigned int)v); }
