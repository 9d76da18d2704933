// oracle/ref_shim/optix.h  --  TEST INFRASTRUCTURE.
//
// Stand-in for <optix.h>: the handful of types and device calls that the reference's raygen / intersection
// programs and its instance kernel use, backed by one per-ray state struct that oracle/ref_driver.cpp fills.
// Written from what the compiler asks for; no reference text in here.
#pragma once
#include "cuda_runtime.h"

typedef unsigned long long OptixTraversableHandle;
typedef unsigned int OptixVisibilityMask;
enum OptixRayFlags { OPTIX_RAY_FLAG_NONE = 0 };
enum OptixInstanceFlags { OPTIX_INSTANCE_FLAG_NONE = 0 };

struct OptixInstance {
    float transform[12]; // 3x4, row major, object to world
    unsigned int instanceId;
    unsigned int sbtOffset;
    unsigned int visibilityMask;
    unsigned int flags;
    OptixTraversableHandle traversableHandle;
    unsigned int pad[2];
};

// What the OptiX runtime knows about the ray whose program is running.
struct EgrShimRay {
    unsigned int payload[8];
    float3 object_origin, object_direction; // the ray in the space of the instance being tested
    unsigned int instance_index;
    uint3 launch_index, launch_dimensions;
};
extern EgrShimRay egr_shim_ray;

#define EGR_SHIM_PAYLOAD(i)                                                              \
    inline unsigned int optixGetPayload_##i() { return egr_shim_ray.payload[i]; }       \
    inline void optixSetPayload_##i(unsigned int v) { egr_shim_ray.payload[i] = v; }
EGR_SHIM_PAYLOAD(0)
EGR_SHIM_PAYLOAD(1)
EGR_SHIM_PAYLOAD(2)
EGR_SHIM_PAYLOAD(3)
EGR_SHIM_PAYLOAD(4)
EGR_SHIM_PAYLOAD(5)
EGR_SHIM_PAYLOAD(6)
EGR_SHIM_PAYLOAD(7)
#undef EGR_SHIM_PAYLOAD

inline float3 optixGetObjectRayOrigin() { return egr_shim_ray.object_origin; }
inline float3 optixGetObjectRayDirection() { return egr_shim_ray.object_direction; }
inline unsigned int optixGetInstanceIndex() { return egr_shim_ray.instance_index; }
inline uint3 optixGetLaunchIndex() { return egr_shim_ray.launch_index; }
inline uint3 optixGetLaunchDimensions() { return egr_shim_ray.launch_dimensions; }

// Supplied by the driver.
void optixTraverse(OptixTraversableHandle handle, float3 ray_origin, float3 ray_direction, float tmin, float tmax, float ray_time,
                   OptixVisibilityMask visibility_mask, unsigned int ray_flags, unsigned int sbt_offset, unsigned int sbt_stride,
                   unsigned int miss_sbt_index, unsigned int &p0, unsigned int &p1, unsigned int &p2, unsigned int &p3, unsigned int &p4,
                   unsigned int &p5, unsigned int &p6, unsigned int &p7);
OptixTraversableHandle optixGetInstanceTraversableFromIAS(OptixTraversableHandle ias, unsigned int instance_index);
const float4 *optixGetInstanceTransformFromHandle(OptixTraversableHandle handle);
const float4 *optixGetInstanceInverseTransformFromHandle(OptixTraversableHandle handle);
