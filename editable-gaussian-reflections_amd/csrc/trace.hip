// The hot path: __raygen__rg + __intersection__gaussian + forward_pass + backward_pass of the reference
// (shaders.cu:9-173, forward_pass.cu:3-155, backward_pass.cu:3-222) as hand-written HIP kernels for gfx950.
//
// Structure (MI355X-first; nothing here is a translation of the OptiX pipeline; DESIGN.md 4 has the measurements):
//   * one wave64 = one 8x8 pixel tile, one lane = one ray; PERSISTENT waves pull tiles from 8 XCD-affine atomic queues
//     (ragged per-ray work: 1..1000s of candidates); waves never wait on each other (no workgroup barrier after the first instruction);
//   * a tile runs through ALL its steps in one go (k_forward_chain: trace, step epilogue, trace, ...; k_backward_chain), so
//     a launch pays the tail of its heaviest tile once per chain, not once per step. The per-step source lives in
//     forward_task.inc / backward_chain.hpp (backward_step) / egr_epilogue.hpp. Per-ray state lives in a task-linear SoA buffer (fully coalesced);
//   * the 8-wide BVH (128-B line-sized nodes, 16-bit child boxes) is walked by PRIMARY tiles as one FRUSTUM (all 64 rays leave the camera
//     origin: one interval test per child slot for the whole tile, eight nodes per iteration; the leaves found are evaluated one after
//     the other, records through the scalar cache, every lane for its own ray) and by BOUNCE tiles as PAIRS (one wave-wide LIFO of
//     (ray, node) pairs and one buffer of (ray, leaf) pairs in LDS: lane m of group g tests child slot m of the g-th popped node, ballots
//     compact the hits, and 64 leaf pairs at a time are evaluated with one lane per pair) - pair_walk below, frustum walk in forward_task.inc;
//   * the forward chain exists as single-wave workgroups and as TEAMS of waves with a shared LDS in which waves without tiles walk pairs
//     their team mates offer (egr_set_team_help, on by default: several waves on one heavy tile - the tail of every launch, most of an under-filled rank's);
//   * the reference's global per-pixel linked list (one same-address atomic per candidate, 36 B entries, pointer chasing)
//     is replaced by a per-resident-wave candidate scratch, one contiguous run per lane ([lane][k]) with bump-allocated
//     extension blocks for the rare long list; it is reused tile after tile;
//   * depth ordering = strict-successor selection in batches of 8 (sorted insertion in registers, stable on ties);
//     semantically the reference's 16-at-a-time k-buffer (forward_pass.cu:55-137) INCLUDING its batch-boundary tie drop (Q3: the tie
//     continuation is switched off at every second batch boundary, forward_task.inc);
//   * composited hits needed by the backward pass go to an arena in 8-row blocks (one atomic per 8 rows per WAVE instead
//     of one per hit per lane), chained newest->oldest, which is the order backward walks;
//   * backward recomputes the local hit point from the snapshot transform instead of storing it. Primary tiles sum their
//     contributions per gaussian in an LDS hash table (DPP neighbour pre-reduction first); whatever leaves the wave - a
//     bounce hit, a flushed table slot - is added to its gaussian's position-ordered gradient row by SIXTEEN LANES PER
//     RECORD (one 64-B non-returning atomic request instead of 15 scattered ones; wide_add_wave); k_grad_gather scatters
//     the rows to the reference's gradient tensors.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <utility>
#include <vector>

#define EGR_CONTRACT_AFTER_EPILOGUE
#include "egr_diag.hpp"
#include "egr_epilogue.hpp" // (includes egr_state.hpp) the step epilogue, for the fused per-tile chain

#ifndef EGR_GPOP
#define EGR_GPOP 5 // pair walk: a walk batch pops up to 8 x EGR_GPOP (ray, node) pairs, EGR_GPOP per lane group (5 since the loop is instantiated per decode: 62 -> 41 spilled VGPRs; before that 4 was best)
#endif
#define EGR_WALK_MAX_LEAVES (8 * EGR_GPOP * EGR_WIDTH) // leaf pairs one walk batch can add
#define EGR_LBUF (64 + 2 * EGR_WALK_MAX_LEAVES) // (an evaluation batch and a walk batch are issued together: room for two walk batches' leaves)
#ifndef EGR_FPOP
#define EGR_FPOP 2 // frustum walk: 8 x EGR_FPOP nodes per iteration (two interleaved same-box pairs: forward chain 3.80-3.87 against 3.92-3.95 ms dense-init; 3 and 4 no further - and the ray table holds the origins of at most 64 + 8 x 2 x 8 buffered leaves: a static_assert says so)
#endif
#ifndef EGR_PSTK
#define EGR_PSTK 512 // pair-stack entries kept in LDS
#endif

namespace {

// XCD-affine persistent scheduling: the task range is cut into 8 contiguous chunks (contiguous image bands), one
// queue head per chunk. A wave first drains the chunk of "its" XCD (workgroup b is observed to run on XCD b % 8;
// used for speed only, any placement is correct), then steals from the others. Each XCD's private 4 MiB L2 then
// holds one band's BVH nodes / Gaussian records instead of the whole frame's, and the single shared head no
// longer serialises 6144 pullers (microarch guide, "dequeue": shard the head per XCD above 64 pullers).
EGR_DI uint32_t wave_next_task(uint32_t *heads, uint32_t num_tasks, uint32_t &cur_q, int lane) {
    const uint32_t chunk = ((num_tasks + 7u) / 8u + 3u) & ~3u;
    for (uint32_t tries = 0; tries < 8u; tries++) {
        const uint32_t q = (cur_q + tries) & 7u;
        const uint32_t beg = q * chunk, end = min(beg + chunk, num_tasks);
        if (beg >= end) continue;
        uint32_t t = 0;
        if (lane == 0) t = atomicAdd(heads + q * EGR_QUEUE_STRIDE, 1u);
        t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
        if (beg + t < end) {
            cur_q = q;
            return beg + t;
        }
    }
    return 0xFFFFFFFFu;
}
EGR_DI uint32_t wave_sum_u32(uint32_t x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += (uint32_t)__shfl_xor((int)x, off);
    return x;
}
EGR_DI uint32_t wave_max_u32(uint32_t x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = max(x, (uint32_t)__shfl_xor((int)x, off));
    return x;
}
EGR_DI void add64(uint32_t *ctrl, int word, uint32_t x) {
    if (x) atomicAdd(reinterpret_cast<unsigned long long *>(ctrl + word), (unsigned long long)x);
}

// T4: primary ray (core/camera.h:17-36). Draw order: jitter.x then jitter.y.
// `view_size` = tanf(vertical_fov / 2) (core/camera.h:21), a launch constant that the compiler cannot hoist out of a task loop (a ~ 150-instruction range
// reduction of a value read through a pointer). The BACKWARD chain evaluates it once in front of its task loop (-1.2 %: 2.37-2.39 against 2.40-2.41 ms, two
// interleaved same-box pairs); the forward chain keeps it per tile: held across its task loop the value costs two more spilled VGPRs and 2 % (2.94-2.99 against
// 2.89-2.90 ms), and read per tile from a word the prologue wrote it measures the same as the tanf (2.85-2.87 against 2.84-2.86 ms) - as long as that word sits on a
// cache line of its own: on the line of the arena's bump counter the one load per tile took the chain from 2.9 to 4.5 ms.
// `w2c` = rows of the world-to-camera rotation: the bound camera's, or a batch view's record (k_batch_cameras).
EGR_DI f3 primary_direction(const DeviceView &v, int ix, int iy, bool jitter, uint32_t &seed, const float view_size, const float *w2c) {
    float aspect_ratio = (float)v.width / (float)v.height;
    float fx = (float)ix, fy = (float)iy;
    if (jitter) {
        float jx = rnd(seed) - 0.5f;
        float jy = rnd(seed) - 0.5f;
        fx += jx;
        fy += jy;
    }
    float y = view_size * (1.0f - 2.0f * (fy + 0.5f) / (float)v.height);
    float x = aspect_ratio * view_size * (2.0f * (fx + 0.5f) / (float)v.width - 1.0f);
    const float *w = w2c; // rows of w2c (= columns of c2w)
    f3 w0 = mk3(w[0], w[1], w[2]), w1 = mk3(w[3], w[4], w[5]), w2 = mk3(w[6], w[7], w[8]);
    return normalize(w0 * x + w1 * y - w2);
}

// One task of a chain kernel (the backward chain decodes it here; the forward chain's loop, forward_chain.inc, spells the same out). BATCH (the frames of egr_render_views, the views of egr_train_views): the task index is
// ((macro-tile group) * batch_frames + frame) << task_shift | sub-task - the frames of one macro tile are adjacent, so the samples of a tile run
// close in time on one XCD (the queue chunks are contiguous task ranges). The tile's pixels come from the base task `tb`, its ray state and its
// rows of the per-task tables from the full index `tq`.
struct ChainTask {
    uint32_t tq;       // full task index: ray state, per-task tables
    uint32_t tb;       // base task: the tile's pixels (== tq outside a batch)
    uint32_t bframe;   // (BATCH) batch frame index of this task
    const float *bcam; // (BATCH) its view's camera record
    bool last_frame;   // (stats / random_seeds are "last launch wins" stores: a batch's last frame only)
};
template <bool BATCH> EGR_DI ChainTask decode_task(const DeviceView &v, const uint32_t tq) {
    ChainTask t{tq, tq, 0u, nullptr, true};
    if constexpr (BATCH) {
        t.tb = batch_base_task(v, tq);
        t.bframe = v.batch_frame0 + (tq >> v.task_shift) % v.batch_frames;
        t.bcam = v.batch_cams + (size_t)(t.bframe / v.batch_spv) * EGR_BATCH_CAM_FLOATS;
        t.last_frame = t.bframe == v.batch_last_frame;
    }
    return t;
}
// The primary ray of pixel `tg` of a task: origin, direction and the seed after the jitter draws. The backward regenerates it from the seed
// instead of reading a stored copy (backward_chain.hpp: output_gradients); forward_task.inc R1 is the same sequence. `view_size`: see primary_direction (a batch reads its view's record).
struct PrimaryRay {
    f3 ro, rd;
    uint32_t seed;
};
template <bool BATCH> EGR_DI PrimaryRay primary_ray(const DeviceView &v, const TaskGeom &tg, const ChainTask &t, const float view_size) {
    PrimaryRay r;
    if constexpr (BATCH) { // frame f of a batch: the f-th of the sequential launches would see total_num_calls + f + 1 (its prologue adds 1)
        r.seed = tea4(tg.pixel_id, (uint32_t)*v.meta.total_num_calls + t.bframe + 1u);
        r.ro = mk3(t.bcam[0], t.bcam[1], t.bcam[2]);
        r.rd = primary_direction(v, tg.px, tg.py, *v.cfg.jitter_primary_rays != 0, r.seed, t.bcam[12], t.bcam + 3);
    } else {
        r.seed = tea4(tg.pixel_id, (uint32_t)*v.meta.total_num_calls); // shaders.cu:88
        r.ro = mk3(v.cam.origin[0], v.cam.origin[1], v.cam.origin[2]);
        r.rd = primary_direction(v, tg.px, tg.py, *v.cfg.jitter_primary_rays != 0, r.seed, view_size, v.cam.rotation_w2c);
    }
    return r;
}

// The geometry of one (ray, gaussian) pair - object-space ray, closest-approach point, the two rejections that only need those
// (shaders.cu:19-20, 36, 41-51) - in ONE function shared by the forward's candidate test and the backward's recomputation (bit-identical
// t and u on both sides), with fused multiply-adds (nvcc's default for the reference too; the CPU oracle evaluates unfused, -ffp-contract=off).
// Which products of `a b + c d + e f` are fused is the compiler's choice PER CALL SITE (it differs between a uniform and a per-lane origin, and between
// two instantiations of one template), while the forward's primary tiles, its pair walk - owner's and helpers' copies - and the backward's
// recomputation must agree to the bit: the fusion is spelled out (the pattern the compiler applied to these expressions in rounds 1-5:
// fma(e, f, fma(a, b, c d))) and the functions themselves are compiled without contraction.
#pragma clang fp contract(off)
EGR_DI float egr_dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return __builtin_fmaf(az, bz, __builtin_fmaf(ax, bx, ay * by));
}
EGR_DI float egr_madd(float a, float b, float c) { // a b + c
    return __builtin_fmaf(a, b, c);
}
EGR_DI float egr_gaussian_sq(float sq, float exp_power) { // eval_gaussian_sq (kernel.cu:8-12) with the division by the launch constant 2p spelled out: its reciprocal is loop-invariant
    const float two_p = 2.0f * exp_power;
    return expf(egr_div_rn(-pow_exp(sq, exp_power), two_p, egr_rcp_refined(two_p)));
}
// (the object-space ORIGIN of a ray is the same for every ray that leaves one point: primary tiles compute it once per leaf, forward_task.inc)
EGR_DI f3 object_origin(const float4 &w0, const float4 &w1, const float4 &w2, const f3 &o) {
    f3 lo;
    lo.x = egr_dot3(w0.x, w0.y, w0.z, o.x, o.y, o.z) + w0.w, lo.y = egr_dot3(w1.x, w1.y, w1.z, o.x, o.y, o.z) + w1.w, lo.z = egr_dot3(w2.x, w2.y, w2.z, o.x, o.y, o.z) + w2.w;
    return lo;
}
EGR_DI void candidate_geometry_from(const float4 &w0, const float4 &w1, const float4 &w2, const f3 &lo, const f3 &d, f3 &ld, f3 &dhat, float &t, f3 &u, bool &behind,
                                    bool &outside) {
    ld.x = egr_dot3(w0.x, w0.y, w0.z, d.x, d.y, d.z), ld.y = egr_dot3(w1.x, w1.y, w1.z, d.x, d.y, d.z), ld.z = egr_dot3(w2.x, w2.y, w2.z, d.x, d.y, d.z);
    const float norm = egr_sqrt_rn(egr_dot3(ld.x, ld.y, ld.z, ld.x, ld.y, ld.z)); // :41
    const float rr = egr_rcp_refined(norm);
    const float inv = egr_div_rn(1.0f, norm, rr);
    dhat.x = ld.x * inv, dhat.y = ld.y * inv, dhat.z = ld.z * inv;          // :42
    const float tl = egr_dot3(-lo.x, -lo.y, -lo.z, dhat.x, dhat.y, dhat.z); // :43
    t = egr_div_rn(tl, norm, rr);                                           // :44
    u.x = egr_madd(tl, dhat.x, lo.x), u.y = egr_madd(tl, dhat.y, lo.y), u.z = egr_madd(tl, dhat.z, lo.z); // :45
    behind = egr_dot3(lo.x, lo.y, lo.z, ld.x, ld.y, ld.z) > 0.0f;           // :36
    outside = egr_dot3(u.x, u.y, u.z, u.x, u.y, u.z) > 1.0f;                // :48-49
}
EGR_DI void candidate_geometry(const float4 &w0, const float4 &w1, const float4 &w2, const f3 &o, const f3 &d, f3 &lo, f3 &ld, f3 &dhat, float &t, f3 &u,
                               bool &behind, bool &outside) {
    lo = object_origin(w0, w1, w2, o);
    candidate_geometry_from(w0, w1, w2, lo, d, ld, dhat, t, u, behind, outside);
}
#pragma clang fp contract(fast)
// Wave-uniform node fetch: constant address space + uniform index => one s_load_dwordx8 through the scalar cache
// (the tree is read-only for the whole launch) instead of a 64-lane vector load.
typedef float egr_v8f __attribute__((ext_vector_type(8)));
EGR_DI void load_node_uniform(const float4 *nodes, uint32_t un, float4 &n0, float4 &n1) {
#if defined(__HIP_DEVICE_COMPILE__)
    const __attribute__((address_space(4))) egr_v8f *p = (const __attribute__((address_space(4))) egr_v8f *)nodes;
    const egr_v8f x = p[un];
    n0 = make_float4(x[0], x[1], x[2], x[3]);
    n1 = make_float4(x[4], x[5], x[6], x[7]);
#else
    n0 = nodes[2 * un], n1 = nodes[2 * un + 1];
#endif
}
typedef float egr_v4f __attribute__((ext_vector_type(4)));
EGR_DI float4 load_f4_uniform(const float4 *base, uint32_t idx) { // idx must be wave-uniform
#if defined(__HIP_DEVICE_COMPILE__)
    const egr_v4f x = ((const __attribute__((address_space(4))) egr_v4f *)base)[idx];
    return make_float4(x[0], x[1], x[2], x[3]);
#else
    return base[idx];
#endif
}
EGR_DI uint4 load_u4_uniform(const uint4 *base, uint32_t idx) { // idx must be wave-uniform
#if defined(__HIP_DEVICE_COMPILE__)
    typedef uint32_t egr_v4u __attribute__((ext_vector_type(4)));
    const egr_v4u x = ((const __attribute__((address_space(4))) egr_v4u *)base)[idx];
    return make_uint4(x[0], x[1], x[2], x[3]);
#else
    return base[idx];
#endif
}
// Segment [tmin,tmax] vs a quantised child box in the frame's cell coordinates: plane distance = fma(cell, invq, ncq)
// with invq = 1/(d*scale), ncq = -origin_cell*invq. Cells 0 / 65535 are the out-of-frame sentinels (-inf / +inf).
// The fused form moves a plane by < 0.01 cell (boxes carry a full extra cell each side); for an exactly axis-parallel
// ray both products are inf and the axis drops out (conservative).
// The interval part of the slab test: [max of the per-axis entries, min of the per-axis exits] clipped to [tmin, tmax].
EGR_DI bool slab_clip(float ax, float bx, float ay, float by, float az, float bz, float tmin, float tmax) {
    const float t0 = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), tmin));
    const float t1 = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fminf(fmaxf(az, bz), tmax));
    return t0 <= t1;
}
EGR_DI bool qslab_hit(uint4 q, f3 invq, f3 ncq, float tmin, float tmax) {
    const uint32_t lx = q.x & 0xFFFFu, ly = q.x >> 16, lz = q.y & 0xFFFFu, hx = q.y >> 16, hy = q.z & 0xFFFFu, hz = q.z >> 16;
    const float flx = lx == 0u ? -3.0e38f : (float)lx, fly = ly == 0u ? -3.0e38f : (float)ly, flz = lz == 0u ? -3.0e38f : (float)lz;
    const float fhx = hx == 65535u ? 3.0e38f : (float)hx, fhy = hy == 65535u ? 3.0e38f : (float)hy, fhz = hz == 65535u ? 3.0e38f : (float)hz;
    const float ax = fmaf(flx, invq.x, ncq.x), bx = fmaf(fhx, invq.x, ncq.x);
    const float ay = fmaf(fly, invq.y, ncq.y), by = fmaf(fhy, invq.y, ncq.y);
    const float az = fmaf(flz, invq.z, ncq.z), bz = fmaf(fhz, invq.z, ncq.z);
    return slab_clip(ax, bx, ay, by, az, bz, tmin, tmax);
}
// Same test when no box of the tree left the build frame (the common case; DeviceView::out_of_frame == 0): no sentinels.
EGR_DI bool qslab_hit_inframe(uint4 q, f3 invq, f3 ncq, float tmin, float tmax) {
    const float flx = (float)(q.x & 0xFFFFu), fly = (float)(q.x >> 16), flz = (float)(q.y & 0xFFFFu);
    const float fhx = (float)(q.y >> 16), fhy = (float)(q.z & 0xFFFFu), fhz = (float)(q.z >> 16);
    const float ax = fmaf(flx, invq.x, ncq.x), bx = fmaf(fhx, invq.x, ncq.x);
    const float ay = fmaf(fly, invq.y, ncq.y), by = fmaf(fhy, invq.y, ncq.y);
    const float az = fmaf(flz, invq.z, ncq.z), bz = fmaf(fhz, invq.z, ncq.z);
    return slab_clip(ax, bx, ay, by, az, bz, tmin, tmax);
}
EGR_DI float4 fetch_a2(const float4 *p) { return *p; }
EGR_DI float4 fetch_a2(float4 v) { return v; }
// OptiX's instance test restated: segment [tmin,tmax] of the object-space ray vs the unit cube.
EGR_DI bool hits_unit_cube(f3 lo, f3 ld, float tmin, float tmax) {
    f3 inv = mk3(__builtin_amdgcn_rcpf(ld.x), __builtin_amdgcn_rcpf(ld.y), __builtin_amdgcn_rcpf(ld.z)); // v_rcp_f32, 1 ulp
    float t0 = tmin, t1 = tmax;
    bool ok = true;
#define EGR_AXIS(c)                                                            \
    if (ld.c != 0.0f) {                                                        \
        float a = (-1.0f - lo.c) * inv.c, b = (1.0f - lo.c) * inv.c;           \
        t0 = fmaxf(t0, fminf(a, b));                                           \
        t1 = fminf(t1, fmaxf(a, b));                                           \
    } else if (lo.c < -1.0f || lo.c > 1.0f)                                    \
        ok = false;
    EGR_AXIS(x) EGR_AXIS(y) EGR_AXIS(z)
#undef EGR_AXIS
    return ok && t0 <= t1;
}

// The same test with IEEE divisions, operation for operation what the CPU oracle evaluates (exact-statistics build only).
EGR_DI bool hits_unit_cube_exact(f3 lo, f3 ld, float tmin, float tmax) {
    float t0 = tmin, t1 = tmax;
    bool ok = true;
#define EGR_AXIS(c)                                                            \
    if (ld.c != 0.0f) {                                                        \
        float a = (-1.0f - lo.c) / ld.c, b = (1.0f - lo.c) / ld.c;             \
        t0 = fmaxf(t0, fminf(a, b));                                           \
        t1 = fminf(t1, fmaxf(a, b));                                           \
    } else if (lo.c < -1.0f || lo.c > 1.0f)                                    \
        ok = false;
    EGR_AXIS(x) EGR_AXIS(y) EGR_AXIS(z)
#undef EGR_AXIS
    return ok && t0 <= t1;
}

// ---------------------------------------------------------------------------------------------------------
// forward chain: teams, the candidate test and the pair walk
// ---------------------------------------------------------------------------------------------------------
// A workgroup of the forward chain is a TEAM of EGR_TEAM waves. Every wave still owns its tiles alone (its own queue pulls, stack,
// leaf buffer, ray table, candidate scratch: waves never wait for each other while there are tiles), but the LDS is shared, and that
// is what lets SEVERAL WAVES WORK ON ONE HEAVY TILE: a wave that finds the task queue empty - or waits for the helpers of its own walk -
// looks for OFFERS, and a walking wave whose pair stack is long while a team mate looks for work puts every other pair of the lower part
// of it (up to EGR_BOX pairs) on offer. The taker walks those pairs on its own stack and leaf buffer against the OWNER's ray table, its
// accepted candidates take slots of the owner's lists through the owner's LDS counters - exactly what the owner would have done with
// them, in another order (the list order of a ray is an implementation matter) - and it may pass part of them on. A rank
// of an 8-way partition has one tile per wave slot and its launch lasts as long as its heaviest tile's chain. On by default
// (egr_team_help_on) - a ray's list order depends on timing, which no output sees except through the order of EXACT depth ties.
#ifndef EGR_TEAM
#define EGR_TEAM 16 // waves per workgroup of the forward chain's team build: the chain exists twice, as teams of this size for launches with
                    // egr_set_team_help(1) and as single-wave workgroups for all others (a team's LDS stays allocated until its last wave
                    // leaves, which costs a whole image 3 % of the chain when nobody helps; 16 = all the waves of a CU can help each other:
                    // rank 0 of an emulated 8-way partition, forward chain 1.60-1.65 ms against 1.66-1.87 with 4 and 1.79 without help)
#endif
#ifndef EGR_BOX
#define EGR_BOX 128 // (ray, node) pairs one offer holds
#endif
#ifndef EGR_DONATE_MIN
#define EGR_DONATE_MIN 96 // a walking wave offers half of its stack from this height on (48 ... 128 make no difference: sweeps r5k)
#endif
#define EGR_BOX_CLAIMED 0x80000000u
#define EGR_EXT_LOCKED (EGR_EXT_NONE - 2u) // a wave of the team is fetching this ray's extension block right now

// The waves of a team run independently, so the kernel has NO workgroup barrier. Within one wave LDS instructions execute in program
// order (a lane reads what another lane of its wave stored by an earlier instruction): all a wave needs between phases that exchange
// data through LDS is that the compiler keeps the order.
EGR_DI void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// (volatile accesses keep their generic address space - the compiler would emit flat_load / flat_store for LDS words - so the cast names LDS)
typedef __attribute__((address_space(3))) uint32_t egr_lds_u32;
EGR_DI uint32_t lds_peek(const uint32_t *p) { return *(const volatile egr_lds_u32 *)p; }
EGR_DI void lds_poke(uint32_t *p, uint32_t x) { *(volatile egr_lds_u32 *)p = x; }
EGR_DI uint32_t uniform_u32(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }

struct FwdConst { // launch constants of a forward wave
    float exp_power, transmittance_threshold, backfacing_max_dist, backfacing_thr, far_plane;
    int num_bounces;
    bool sentinels;
    const float4 *__restrict__ app;
    const uint4 *__restrict__ wnodes;
};
// egr_object_masks (k_forward_objects): what the primary step composites instead of the appearance, and where the tile's end writes it. A kernel argument of
// that kernel alone (not part of DeviceView); the other three chain kernels hold an empty one that no code of theirs reads.
struct ObjectQuery {
    const uint32_t *pos_bits; // [n] membership word per RECORD (sorted position), bit j = the row belongs to the j-th REQUESTED object (k_object_bits)
    uint32_t num_bits;        // K requested objects, 1 .. 32
    float *masks;             // [K][H][W]
    uint32_t *hit;            // [H][W] or NULL
    int32_t *top;             // [H][W] or NULL
};
struct ObjectBitList { // the requested selection bits in output order (a kernel argument: no upload)
    uint8_t bit[32];
};
struct WalkShared { // one wave's LDS
    uint32_t pstk[EGR_PSTK];  // (ray << 26 | wide node); entries beyond EGR_PSTK spill to the wave's global column
    uint32_t lbuf[EGR_LBUF];  // (ray << 26 | record) awaiting evaluation; a walk batch adds <= 8 GPOP x 8 and only runs when that fits
    float4 rayp[EGR_WAVE][3]; // per ray: (o.xyz, d.x) (d.yz, invq.xy) (invq.z, ncq.xyz)
    uint32_t gcnt[EGR_WAVE], gtrav[EGR_WAVE]; // accepted / counted candidates per ray
    uint32_t gext[EGR_WAVE];  // extension block of a ray's candidate list (EGR_EXT_NONE: none)
    uint32_t wc[4 * EGR_NSTEPS]; // this wave's ray / candidate / composited / accepted counts per step
};
template <int TEAM> struct TeamShared {
    uint32_t done;                 // waves of the team that found the task queue empty (they only help from then on)
    uint32_t hungry;               // waves looking for an offer right now (out of tiles, or waiting for the helpers of their own walk)
    uint32_t box_count[TEAM];  // the offer of wave w: pairs | rays' owner << 16 (0: none; EGR_BOX_CLAIMED set: being copied out)
    uint32_t busy[TEAM];       // other waves that hold pairs of wave w's current walk (a wave announces itself here BEFORE it claims an offer)
    uint32_t ctx[TEAM][5];     // the walk wave w's offers belong to: step | seg << 8, seg_lo, seg_hi, near plane, the wave whose rays these are
    uint32_t box[TEAM][EGR_BOX];
};
struct WalkStats { // diagnostic builds (egr_diag.hpp: EGR_WALK)
    uint32_t visits = 0, leafhits = 0, inner = 0, outer = 0;
    uint32_t offers = 0, tall = 0; // team: offers made, walk batches that left the stack at EGR_DONATE_MIN pairs or more
};

// R2 for one (ray, gaussian) pair given the gaussian's W rows and live (.., opacity, sigma) record (shaders.cu:9-75).
// `prim` is the gaussian's SORTED POSITION (record index), not its id.
// returns 0: not this segment's / not met by the reference, 1: counted and rejected, 2: accepted (t, alpha valid), 3: response point outside
// the ellipsoid (rejected; counted only by the exact-statistics build). What a DEFAULT launch counts (num_traversed_per_pixel,
// egr_counters.candidates) is a property of the ray and the gaussian alone, not of how the tree was walked: the candidates whose response
// point lies INSIDE the gaussian's ellipsoid on the ray's segment - a subset of the reference's intersection-program invocations
// (every instance whose CUBE the segment overlaps, shaders.cu:33), which the exact-statistics build counts (egr_set_exact_stats).
// SEG0: the caller's copy of the loop only runs for segment 0 (the hot case: no runtime segment dispatch).
template <bool CUBE, bool SEG0, class A2>
EGR_DI int test_candidate(const FwdConst &fc, int step, int seg, float near_plane, const f3 &o, const f3 &d, uint32_t prim, const float4 &w0, const float4 &w1,
                          const float4 &w2, A2 a2src, float &t, float &alpha, const f3 *lo_pre = nullptr) {
    const float far_plane = fc.far_plane;
    f3 lo, ld, dhat, u;
    bool behind, outside;
    if (lo_pre != nullptr) { // (primary tiles: the object-space origin was computed once per leaf - the same expression, object_origin)
        lo = *lo_pre;
        candidate_geometry_from(w0, w1, w2, lo, d, ld, dhat, t, u, behind, outside);
    } else {
        candidate_geometry(w0, w1, w2, o, d, lo, ld, dhat, t, u, behind, outside); // :19-20, :36, :41-51
    }
    if constexpr (CUBE) {
        // exact-statistics build: the tree bounds the instance cubes, one walk over [tmin,tmax] meets every instance OptiX
        // would invoke the intersection program for; the cube test is the oracle's (IEEE division)
        if (!hits_unit_cube_exact(lo, ld, near_plane, far_plane)) return 0;
    } else {
        // each candidate is owned by exactly one of the three walked segments (forward_task.inc): counted / accepted once
        if constexpr (SEG0) {
            if (!(t >= near_plane && t <= far_plane)) return 0;
        } else if (!(seg == 0 ? (t >= near_plane && t <= far_plane) : seg == 1 ? (t < near_plane) : (t > far_plane))) return 0;
        // OptiX only invokes the intersection program when the instance's unit cube overlaps [tmin,tmax]. A response point
        // inside the unit sphere AND on the segment (segment 0) is itself a point of cube and segment, so the cube test is
        // implied for everything segment 0 ACCEPTS; of the hits it rejects, those behind the origin or back-facing are counted without
        // asking whether the reference would have looked at them, those outside the ellipsoid are not counted at all (default launches
        // count the candidates INSIDE their ellipsoid - include/egr_raytracer.h, egr_set_exact_stats -, the exact-statistics build counts
        // the reference's invocations). Segments 1 / 2 hold the Q1 hits, accepted only if the cube overlaps [tmin,tmax].
        if constexpr (!SEG0)
            if (seg != 0 && !hits_unit_cube(lo, ld, near_plane, far_plane)) return 0;
    }
    if (outside) return CUBE ? 1 : 3;               // :48-51 (the exact-statistics build counts every invocation, shaders.cu:33)
    if (behind) return 1;                           // :36
    if (step != 0 && t < fc.backfacing_max_dist) {  // :54-61 (world normal . object dir)
        const float4 n0 = fc.app[2 * prim], n1 = fc.app[2 * prim + 1]; // raw normal, record order (k_live)
        f3 gn = mk3(n0.w, n1.x, n1.y);
        if (sqrtf(egr_dot3(gn.x, gn.y, gn.z, gn.x, gn.y, gn.z)) > fc.backfacing_thr && egr_dot3(gn.x, gn.y, gn.z, dhat.x, dhat.y, dhat.z) > 0.0f) return 1;
    }
    const float4 a2 = fetch_a2(a2src);                        // live quarter of the record, only now
    f3 x = u * a2.w;                                          // :64
    float gaussval = egr_gaussian_sq(egr_dot3(x.x, x.y, x.z, x.x, x.y, x.z), fc.exp_power); // :65 (spelled-out fusion: the owner's and a helper's copy of this test agree to the bit)
    alpha = EGR_MAX_ALPHA * gaussval * a2.z;                   // kernel.cu:14-16
    return 2;
}

// Per-ray pre-test of primary tiles (forward_task.inc), before a (ray, gaussian) pair is evaluated at all: the ray against the gaussian's bounding sphere
// (bvh.hip: bsph). staged_sphere runs once per buffered leaf and returns a / rad, the vector from the camera to the centre in units of the PADDED radius;
// ray_misses_sphere runs per (ray, leaf): the line o + t d misses the sphere iff |a x d|^2 > rad^2 |d|^2, i.e. |(a / rad) x d|^2 > |d|^2.
// What a rejection must imply is that test_candidate returns 0 or 3 for the pair (never counted, never appended), i.e. that `outside` as
// candidate_geometry_from computes it in fp32 is true. In exact arithmetic |u| >= (distance of the line from the centre) / s_max, s_max the largest
// semi-axis, so a line that misses the sphere of radius s_max (1 + m) has |u| >= 1 + m. The fp32 |u| differs from that by
//   (a) the rounding of lo = W o + w, a cancellation: <= 3 x 2^-24 (|o|_1 + |centre|_1) in WORLD units on every axis, whatever the scale;
//   (b) the direction dhat = W d / |W d|: every component of W d is rounded to 2^-23 |d| / s_a, against |W d| >= |d| / s_max: an angle of
//       sqrt(3) 2^-23 k, k = s_max / s_min, which moves u = lo - (lo . dhat) dhat by up to |lo| times that;
//   (c) the roundings of tl, of dhat's length and of the three fma of u: about 6 x 2^-24 |lo|.
// Hence m = 0.005 + 1e-6 |lo|_1 (k + 1) (four to five times (b) + (c)), and 1e-6 (|o|_1 + |centre|_1) is added to the radius for (a). The fixed 0.5 %
// alone would stop covering (b) + (c), about 2e-7 |lo| (k + 2), at |lo| (k + 2) of about 2e4: a round gaussian 1e4 of its radii from the camera - a 1e-4
// gaussian at distance 50 is fifty times beyond that, so the pad scales with |lo|. The pre-test's own arithmetic (a = centre - o, the cross product)
// is covered by 2e-6 |a|_1, as in the leaf filter. Only finite evidence rejects: a NaN or an inf on either side keeps the pair.
EGR_DI f3 staged_sphere(const float4 &sp, const float4 &w0, const float4 &w1, const float4 &w2, const f3 &lo, const f3 &o) {
    const f3 a = mk3(sp.x - o.x, sp.y - o.y, sp.z - o.z);
    const float smax = sqrtf(fmaxf(sp.w, 0.0f));                                                                              // (padded by k_instances)
    const float inv_smin = sqrtf(fmaxf(fmaxf(dot(mk3(w0.x, w0.y, w0.z), mk3(w0.x, w0.y, w0.z)), dot(mk3(w1.x, w1.y, w1.z), mk3(w1.x, w1.y, w1.z))),
                                       dot(mk3(w2.x, w2.y, w2.z), mk3(w2.x, w2.y, w2.z)))); // rows of W = columns of R over the scales
    const float lo1 = fabsf(lo.x) + fabsf(lo.y) + fabsf(lo.z);
    const float rad = smax * (1.005f + 1e-6f * lo1 * (smax * inv_smin + 1.0f)) + 2e-6f * (fabsf(a.x) + fabsf(a.y) + fabsf(a.z)) +
                      1e-6f * (fabsf(o.x) + fabsf(o.y) + fabsf(o.z) + fabsf(sp.x) + fabsf(sp.y) + fabsf(sp.z));
    const float ir = sp.w >= 0.0f ? 1.0f / rad : u2f(0x7FC00000u); // (an unusable gaussian: NaN, every pair is kept and the candidate test rejects it as before)
    return mk3(a.x * ir, a.y * ir, a.z * ir);
}
EGR_DI bool ray_misses_sphere(const f3 &an, const f3 &d, float d2) { // an: staged_sphere; d2 = |d|^2
    const f3 c = cross(an, d);
    const float c2 = dot(c, c);
    return c2 > d2 && c2 < __builtin_inff();
}

// One evaluation batch worked off: lane = one (ray, gaussian) pair whose 64-B record (w0..w2 = rows of W, w3 = live quarter) has arrived. The candidate
// test, then an accepted candidate takes a slot of its ray's list through the ray's LDS counter (the run in the wave's scratch, beyond cand_cap ONE
// extension block per ray). Shared by the pair walk of bounce tiles and by the primary tiles' leaf evaluation (forward_task.inc).
template <bool CUBE, bool SEG0>
EGR_DI void pair_eval_append(const DeviceView &v, const FwdConst &fc, WalkShared &rays, const size_t scratch0, const int step, const int seg, const float near_plane, const bool have,
                             const uint32_t er, const uint32_t pidx, const float4 &w0, const float4 &w1, const float4 &w2, const float4 &w3, bool &g_over, WalkStats &st) {
    const int lane = threadIdx.x & (EGR_WAVE - 1);
    (void)lane;
    int res = 0;
    float t = 0.0f, alpha = 0.0f;
    if (have) {
        const float4 q0 = rays.rayp[er][0], q1 = rays.rayp[er][1];
        res = test_candidate<CUBE, SEG0>(fc, step, seg, near_plane, mk3(q0.x, q0.y, q0.z), mk3(q0.w, q1.x, q1.y), pidx, w0, w1, w2, w3, t, alpha);
    }
    EGR_WALK(st.leafhits += have ? 1u : 0u; st.outer += (lane == 0);)
    if (res == 1 || res == 2) atomicAdd(&rays.gtrav[er], 1u);
    uint32_t at = 0u;
    if (res == 2) at = atomicAdd(&rays.gcnt[er], 1u);
    const bool in_ext = res == 2 && at >= v.cand_cap;
    if (res == 2 && !in_ext) {
        const size_t slot = (scratch0 + er) * v.cand_cap + at;
        v.cand_keys[scratch0 * v.cand_cap + ((((size_t)(at >> 2) * EGR_WAVE + er) << 2) + (at & 3u))] = t; // (forward_decl.inc: EGR_KEY_AT of the owner's region)
        v.cand_vals[slot] = make_float2(alpha, u2f(pidx)); // (a pair walk's lists are contiguous runs: forward_decl.inc)
    }
    if (__ballot(in_ext) != 0ull) { // rare: some list outgrew its run - it continues in ONE extension block per ray
        for (;;) { // rays that need a block and have none, one after the other (wave-uniform loop)
            const unsigned long long pend = __ballot(in_ext && lds_peek(&rays.gext[er]) == EGR_EXT_NONE);
            if (pend == 0ull) break;
            const int src = __ffsll((long long)pend) - 1;
            if (lane == src && atomicCAS(&rays.gext[er], EGR_EXT_NONE, EGR_EXT_LOCKED) == EGR_EXT_NONE) { // (a team mate working on the same ray may be faster)
                const uint32_t e = atomicAdd(v.control + CW_EXT_BUMP, 1u);
                lds_poke(&rays.gext[er], e < v.ext_blocks_cap ? e : EGR_EXT_NONE - 1u); // EGR_EXT_NONE - 1 = none left
            }
            wave_sync();
        }
        if (in_ext) {
            uint32_t e = lds_peek(&rays.gext[er]);
            while (e == EGR_EXT_LOCKED) __builtin_amdgcn_s_sleep(1), e = lds_peek(&rays.gext[er]);
            const uint32_t k = at - v.cand_cap;
            if (e < EGR_EXT_NONE - 1u && k < EGR_EXT_BLOCK) {
                v.ext_keys[(size_t)e * EGR_EXT_BLOCK + k] = t;
                v.ext_vals[(size_t)e * EGR_EXT_BLOCK + k] = make_float2(alpha, u2f(pidx));
            } else {
                g_over = true;
            }
        }
    }
}

// ---- pair walk. Work items are PAIRS, not rays: a wave-wide LIFO of (ray, node) pairs and a buffer of (ray, leaf) pairs,
// both in LDS. A walk iteration pops up to 8 x EGR_GPOP pairs; lane m of group g tests child slot m of the g-th popped node
// (one 16-B load per lane = the node's 128-B line per group), hits are compacted with wave-wide ballots: inner children
// back onto the stack, leaves into the leaf buffer. Whenever 64 leaf pairs wait, ONE LANE PER PAIR evaluates them (every
// lane busy, no per-ray open / close, no leaf queue in global memory). Accepted candidates take a slot of their ray's list
// through an LDS counter; the total transmittance is multiplied up from the finished list (its order, like the
// reference's insertion order, is an implementation matter: deterministic for a wave that walks alone).
// The loop exists once per decode of the child boxes (SENT: out-of-frame sentinels or not, wave-uniform for the whole launch) and once more
// for segment 0 without sentinels (SEG0; nearly every walk of a bounce step) - the choice is made once per walk instead of once per slot batch.
// `mine`: stack and leaf buffer of the executing wave; `rays`: ray table, per-ray counters and (through scratch0) candidate lists of the
// wave that OWNS the tile - the same wave unless the pairs were taken from an offer (team_help). The caller enters with `top` pairs on mine.pstk.
template <bool SENT, bool SEG0, bool CUBE, int TEAM>
EGR_DI void pair_walk(const DeviceView &v, const FwdConst &fc, WalkShared &mine, WalkShared &rays, TeamShared<TEAM> &team, const int self, const size_t scratch0,
                      uint32_t *__restrict__ gstk, const int step, const int seg, const float seg_lo, const float seg_hi, const float near_plane, uint32_t top,
                      bool &g_over, WalkStats &st) {
    const int lane = threadIdx.x & (EGR_WAVE - 1);
    const uint32_t m = (uint32_t)lane & 7u, grp = (uint32_t)lane >> 3;
    constexpr uint32_t GSTK_CAP = (uint32_t)EGR_GSTK * EGR_WAVE;
    const uint4 *__restrict__ wnodes = fc.wnodes;
    uint32_t nl = 0u; // wave-uniform height of the leaf buffer (top: of the pair stack)
    uint32_t hungry_seen = 0u;
    for (;;) {
        // One iteration = (up to) one evaluation batch AND one walk batch: the record fetches of the batch of 64 leaf pairs and
        // the node fetches of the popped pairs are issued together, then both are worked off - a tile's critical path is its
        // chain of dependent fetches (every batch needs what the previous one found), so two kinds of work per round trip
        // instead of one shorten it (the walk refills the leaf buffer with ~40 pairs per iteration).
        const bool do_eval = nl >= (uint32_t)EGR_WAVE || (top == 0u && nl > 0u); // wave-uniform
        if (!do_eval && top == 0u) {
            if constexpr (TEAM > 1) {
                // an offer of this wave that nobody took comes back. (One that is being copied out right now is the taker's: it announced
                // itself in busy[rays' owner] before it claimed the offer, and that owner waits for it - forward_task.inc.)
                uint32_t r = 0u;
                if (lane == 0) {
                    const uint32_t c = lds_peek(&team.box_count[self]);
                    if (c != 0u && !(c & EGR_BOX_CLAIMED) && atomicCAS(&team.box_count[self], c, c | EGR_BOX_CLAIMED) == c) r = c;
                }
                r = uniform_u32(r);
                if (r != 0u) {
                    r &= 0xFFFFu;
                    for (uint32_t i = (uint32_t)lane; i < r; i += EGR_WAVE) mine.pstk[i] = team.box[self][i];
                    top = r;
                    wave_sync();
                    if (lane == 0) lds_poke(&team.box_count[self], 0u);
                    continue;
                }
            }
            break;
        }
        // ---------------- issue: evaluation batch (64 (ray, leaf) pairs, one lane each)
        bool have = false;
        uint32_t er = 0u, pidx = 0u;
        float4 w0 = make_float4(0, 0, 0, 0), w1 = w0, w2 = w0, w3 = w0; // the whole 64-B record: rows of W + the live quarter (same line)
        if (do_eval) {
            const uint32_t take = min(nl, (uint32_t)EGR_WAVE);
            nl -= take;
            have = (uint32_t)lane < take;
            const uint32_t pr = mine.lbuf[nl + min((uint32_t)lane, take - 1u)];
            er = pr >> 26, pidx = pr & 0x03FFFFFFu;
            if (have) w0 = v.inst_w[4 * pidx], w1 = v.inst_w[4 * pidx + 1], w2 = v.inst_w[4 * pidx + 2], w3 = v.inst_w[4 * pidx + 3];
        }
        // ---------------- issue: walk batch (pop up to 8 x EGR_GPOP (ray, node) pairs)
        // (a walk batch only runs when the leaf pairs it can add fit the buffer: otherwise this iteration only evaluates)
        const uint32_t npop = nl + (uint32_t)EGR_WALK_MAX_LEAVES <= (uint32_t)EGR_LBUF ? min(top, 8u * (uint32_t)EGR_GPOP) : 0u;
        uint32_t pw[EGR_GPOP];
        uint4 sl_[EGR_GPOP];
        if constexpr (TEAM > 1) hungry_seen = lds_peek(&team.hungry); // (read with the stack: one LDS round trip)
        if (npop != 0u) {
#pragma unroll
            for (int u = 0; u < EGR_GPOP; u++) pw[u] = mine.pstk[min(top - 1u - min(grp + 8u * (uint32_t)u, top - 1u), (uint32_t)EGR_PSTK - 1u)];
            if (top > (uint32_t)EGR_PSTK) { // some popped pairs live in the global spill column (rare; volatile keeps it a global load)
#pragma unroll
                for (int u = 0; u < EGR_GPOP; u++) {
                    const uint32_t e = top - 1u - min(grp + 8u * (uint32_t)u, top - 1u);
                    if (grp + 8u * (uint32_t)u < npop && e >= (uint32_t)EGR_PSTK) pw[u] = *reinterpret_cast<const volatile uint32_t *>(gstk + (e - EGR_PSTK));
                }
            }
#pragma unroll
            for (int u = 0; u < EGR_GPOP; u++) {
                // (a group beyond the popped pairs re-reads the bottom pair's node - a valid entry, the index above is clamped - and is
                // turned into an empty slot: no exec-mask detour around the load)
                sl_[u] = wnodes[(size_t)(pw[u] & 0x03FFFFFFu) * EGR_WIDTH + m];
                if (!(grp + 8u * (uint32_t)u < npop)) sl_[u].w = EGR_EMPTY_SLOT;
            }
            top -= npop;
            EGR_WALK(st.visits += (m == 0u) ? min(npop > grp ? (npop - grp + 7u) / 8u : 0u, (uint32_t)EGR_GPOP) : 0u; st.inner += (lane == 0);)
        }
        wave_sync(); // the reads of both buffers above come before the pushes below
        // ---------------- work off: evaluation batch
        if (do_eval) pair_eval_append<CUBE, SEG0>(v, fc, rays, scratch0, step, seg, near_plane, have, er, pidx, w0, w1, w2, w3, g_over, st);
        // ---------------- work off: walk batch
        if (npop != 0u) {
#pragma unroll
            for (int u = 0; u < EGR_GPOP; u++) {
                const uint32_t rtag = pw[u] & 0xFC000000u; // the pair's ray, in place
                const float4 q1 = rays.rayp[pw[u] >> 26][1], q2 = rays.rayp[pw[u] >> 26][2];
                const uint4 sl = sl_[u];
                // (masks built on the scalar side: one ballot of the box test, one of the leaf bit; an unpopped slot is an empty slot)
                const bool hit = (SENT ? qslab_hit(sl, mk3(q1.z, q1.w, q2.x), mk3(q2.y, q2.z, q2.w), seg_lo, seg_hi) : qslab_hit_inframe(sl, mk3(q1.z, q1.w, q2.x), mk3(q2.y, q2.z, q2.w), seg_lo, seg_hi)) & (sl.w != EGR_EMPTY_SLOT);
                const bool leaf = (int)sl.w < 0;
                const unsigned long long hm = __builtin_amdgcn_ballot_w64(hit), lm = __builtin_amdgcn_ballot_w64(leaf);
                const unsigned long long im = hm & ~lm, fm = hm & lm;
                const uint32_t at = top + __builtin_amdgcn_mbcnt_hi((uint32_t)(im >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)im, 0u));
                if (top + (uint32_t)EGR_WAVE <= (uint32_t)EGR_PSTK) { // wave-uniform: every push of this batch stays in the LDS part (the usual case)
                    if (hit & !leaf) mine.pstk[at] = rtag | sl.w;
                    top += (uint32_t)__popcll(im);
                } else {
                    if (hit & !leaf) {
                        if (at < (uint32_t)EGR_PSTK) mine.pstk[at] = rtag | sl.w;
                        else if (at - EGR_PSTK < GSTK_CAP) gstk[at - EGR_PSTK] = rtag | sl.w;
                        else g_over = true;
                    }
                    top = min(top + (uint32_t)__popcll(im), (uint32_t)EGR_PSTK + GSTK_CAP);
                }
                if (hit & leaf) mine.lbuf[nl + __builtin_amdgcn_mbcnt_hi((uint32_t)(fm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)fm, 0u))] = rtag | (sl.w & ~EGR_LEAF_FLAG);
                nl += (uint32_t)__popcll(fm);
            }
        }
        wave_sync();
        EGR_WALK(st.tall += (lane == 0 && top >= (uint32_t)EGR_DONATE_MIN) ? 1u : 0u;)
        if constexpr (TEAM > 1) {
            // a team mate looks for work and this stack is long: its lower half goes on offer
            if (uniform_u32(hungry_seen) != 0u && top >= (uint32_t)EGR_DONATE_MIN && top <= (uint32_t)EGR_PSTK && uniform_u32(lds_peek(&team.box_count[self])) == 0u) {
                // EVERY OTHER pair of the lower part of the stack goes, the rest moves down. Both halves then hold subtrees of every size (the
                // bottom holds the pairs nearest the root, i.e. the largest subtrees still to walk, the top the crumbs of the subtree the wave
                // is in). Measured on rank 0 of an emulated 8-way partition: offers from the top shortened the heaviest walk by a quarter at
                // best; offers of the bottom half left the owner waiting for its helpers for as long as its own half had taken.
                const uint32_t give = min(top >> 1, (uint32_t)EGR_BOX);
                for (uint32_t base = 0u; base < top; base += EGR_WAVE) {
                    const uint32_t i = base + (uint32_t)lane;
                    const uint32_t x = mine.pstk[min(i, (uint32_t)EGR_PSTK - 1u)];
                    wave_sync();
                    if (i < 2u * give) {
                        if (i & 1u) team.box[self][i >> 1] = x;
                        else mine.pstk[i >> 1] = x;
                    } else if (i < top) mine.pstk[i - give] = x;
                }
                top -= give;
                wave_sync();
                if (lane == 0) lds_poke(&team.box_count[self], give | (lds_peek(&team.ctx[self][4]) << 16));
                EGR_WALK(st.offers += (lane == 0);)
            }
        }
    }
}

// A turn of a wave that looks for work: take an offer of a team mate and walk it - on this wave's own stack and leaf buffer, against the
// ray table, per-ray counters and candidate lists of the wave whose rays the pairs belong to (ONE generic instance of pair_walk:
// sentinel-aware, any segment). Returns false when there was no offer. The caller counts itself in team.hungry while it looks.
template <bool CUBE, int TEAM> EGR_DI bool team_help(const DeviceView &v, const FwdConst &fc, WalkShared *wsh, TeamShared<TEAM> &team, const int wv, const uint32_t slot0, bool &g_over) {
    const int lane = threadIdx.x & (EGR_WAVE - 1);
    for (int dlt = 1; dlt < TEAM; dlt++) {
        const int w = (wv + dlt) % TEAM;
        uint32_t k = 0u, o = 0u;
        if (lane == 0) {
            const uint32_t c = lds_peek(&team.box_count[w]);
            if (c != 0u && !(c & EGR_BOX_CLAIMED)) {
                o = (c >> 16) & 0xFFu;
                atomicAdd(&team.busy[o], 1u); // first: the rays' owner must never see "nobody busy" while these pairs are open
                if (atomicCAS(&team.box_count[w], c, c | EGR_BOX_CLAIMED) == c) k = c & 0xFFFFu; // (ctx[w] cannot change while an offer of w is open)
                else atomicSub(&team.busy[o], 1u);
            }
        }
        k = uniform_u32(k);
        if (k == 0u) continue;
        const int owner = (int)uniform_u32(o);
        if (lane == 0) atomicSub(&team.hungry, 1u);
        WalkShared &mine = wsh[wv];
        for (uint32_t i = (uint32_t)lane; i < k; i += EGR_WAVE) mine.pstk[i] = team.box[w][i];
        const uint32_t c0 = uniform_u32(lds_peek(&team.ctx[w][0])), c1 = uniform_u32(lds_peek(&team.ctx[w][1])), c2 = uniform_u32(lds_peek(&team.ctx[w][2])), c3 = uniform_u32(lds_peek(&team.ctx[w][3]));
        // this wave's own offers (it may pass on part of what it took) describe the same walk; its last offer may still be on its way out
        while (uniform_u32(lds_peek(&team.box_count[wv])) != 0u) __builtin_amdgcn_s_sleep(1);
        if (lane == 0) lds_poke(&team.ctx[wv][0], c0), lds_poke(&team.ctx[wv][1], c1), lds_poke(&team.ctx[wv][2], c2), lds_poke(&team.ctx[wv][3], c3), lds_poke(&team.ctx[wv][4], (uint32_t)owner);
        wave_sync();
        if (lane == 0) lds_poke(&team.box_count[w], 0u); // w may offer the next batch
        const int step = (int)(c0 & 0xFFu), seg = (int)(c0 >> 8);
        const size_t scratch0 = ((size_t)slot0 + (size_t)owner) * EGR_WAVE; // the OWNER's candidate lists
        uint32_t *gstk = v.stack_spill + ((size_t)slot0 + (size_t)wv) * EGR_GSTK * EGR_WAVE; // this wave's own spill column
        WalkStats st;
        pair_walk<true, false, CUBE, TEAM>(v, fc, mine, wsh[owner], team, wv, scratch0, gstk, step, seg, u2f(c1), u2f(c2), u2f(c3), k, g_over, st);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); // the list entries written for the owner
        EGR_WALK(if (lane == 0) atomicAdd(v.control + DG_TEAM_HELPED, 1u), atomicAdd(v.control + DG_TEAM_HELP_ITERS, st.inner);)
        if (lane == 0) atomicSub(&team.busy[owner], 1u), atomicAdd(&team.hungry, 1u);
        return true;
    }
    return false;
}
// ... for as long as `wanted()` says (wave-uniform): the waiting loop of an owner whose walk still has helpers, and of a wave without tiles.
template <bool CUBE, int TEAM, class F> EGR_DI void team_help_while(const DeviceView &v, const FwdConst &fc, WalkShared *wsh, TeamShared<TEAM> &team, const int wv, const uint32_t slot0, bool &g_over, F wanted) {
    const int lane = threadIdx.x & (EGR_WAVE - 1);
    if (!wanted()) return;
    if (lane == 0) atomicAdd(&team.hungry, 1u);
    while (wanted())
        if (!team_help<CUBE, TEAM>(v, fc, wsh, team, wv, slot0, g_over)) __builtin_amdgcn_s_sleep(4);
    if (lane == 0) atomicSub(&team.hungry, 1u);
}

// ---------------------------------------------------------------------------------------------------------
// per-launch prologue: Raytracer::raytrace host part (raytracer.cpp:82-86), on the device, no host sync
// ---------------------------------------------------------------------------------------------------------
// The control-word resets of the one-block (one-wave) prologue kernels, t = threadIdx.x.
// Per launch: the counters [0, CW_RESET_END), the diagnostic words and the lines of the two bump counters [DG_BEGIN, CW_COUNT), then the min / max seeds of DG_STEP_EXIT.
EGR_DI void reset_launch_words(const DeviceView &v, int t) {
    if (t < CW_RESET_END) v.control[t] = 0;
    for (int w = DG_BEGIN + t; w < CW_COUNT; w += (int)blockDim.x) v.control[w] = 0;
    if (t < 12) v.control[DG_STEP_EXIT + t] = ((t & 3) < 2) ? 0xFFFFFFFFu : 0u;
}
// Per chunk of tasks (a single launch is one chunk): fresh task queues of both chains, extension blocks and hit-arena blocks.
EGR_DI void reset_chunk_words(const DeviceView &v, int t) {
    for (uint32_t q = t; q < EGR_QUEUE_WORDS; q += blockDim.x) v.queues[q] = 0;
    if (t == 0) v.control[CW_EXT_BUMP] = 0, v.control[CW_HIT_BUMP] = 0;
}
// The lifetime counters at the end of a call that traced `launches` frames (one thread).
EGR_DI void count_lifetime(const DeviceView &v, uint32_t launches) {
    unsigned long long rays = 0;
    for (int s = 0; s < EGR_NSTEPS; s++) rays += *reinterpret_cast<unsigned long long *>(v.control + CW_RAYS + 2 * s);
    *reinterpret_cast<unsigned long long *>(v.control + CW_LIFE_RAYS) += rays;
    v.control[CW_LIFE_LAUNCHES] += launches;
}
__global__ void k_prologue(DeviceView v, int grads) {
    const int t = threadIdx.x;
    reset_launch_words(v, t);
    reset_chunk_words(v, t);
    if (t == 0) {
        *v.meta.grads_enabled = grads ? 1 : 0;   // metadata.h:29
        *v.meta.total_num_calls += 1;             // metadata.h:30
    }
}
__global__ void k_epilogue(DeviceView v, int grads) {
    // raytracer.cpp:91-93 (the reference adds 1 whenever accumulate_samples is set)
    if (threadIdx.x == 0) {
        if (*v.cfg.accumulate_samples) *v.fb.accumulated_sample_count += 1;
        count_lifetime(v, 1u);
    }
}
// per-launch live record: activated appearance + (opacity, sigma). Reads the CURRENT parameter tensors, like
// the reference's read_* helpers do inside the launch (utils/helpers.cu:10-33), while the transforms in inst_w / inst_m stay
// snapshots of the last update_bvh / rebuild_bvh. Grad launches also refresh the two live quantities of the backward record:
// exp(scale) and the raw quaternion, which the reference's backward reads from the parameter tensors (backward_pass.cu:68-70)
// next to OptiX's snapshot transforms (:75-78).
__global__ void __launch_bounds__(256) k_live(DeviceView v, int grads) {
    uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= v.n) return;
    const egr_gaussians &g = v.g;
    float o = sigmoid_act(g.opacity[i]);
    float sigma = compute_scaling_factor(o, *v.cfg.alpha_threshold, *v.cfg.exp_power);
    const size_t pos = v.pos_of_gid[i]; // stored at the sorted position
    float4 *app = v.app + 2 * pos;
    app[0] = make_float4(relu_act(g.rgb[3 * i]), relu_act(g.rgb[3 * i + 1]), relu_act(g.rgb[3 * i + 2]), g.normal[3 * i]);
    app[1] = make_float4(g.normal[3 * i + 1], g.normal[3 * i + 2], clip01_act(g.f0[3 * i]), clip01_act(g.f0[3 * i + 1]));
    // the 4th quarter of the 64-B test record (rows of W are the first three): what a candidate test needs besides W
    v.inst_w[4 * pos + 3] = make_float4(clip01_act(g.f0[3 * i + 2]), clip01_act(g.roughness[i]), o, sigma);
    if (grads) {
        float4 *im = v.inst_m + 4 * (size_t)i; // (the backward record is kept by id: egr_internal.hpp)
        im[0].w = expf(g.scale[3 * i]), im[1].w = expf(g.scale[3 * i + 1]), im[2].w = expf(g.scale[3 * i + 2]);
        im[3] = reinterpret_cast<const float4 *>(g.rotation)[i];
    }
}

// ---------------------------------------------------------------------------------------------------------
// forward: all bounce steps of every tile of this rank
// ---------------------------------------------------------------------------------------------------------
// The fused per-tile chain: a wave takes a tile through ALL its steps (trace, step epilogue, trace, ...) before it takes the
// next tile. A rank's forward time is then max over tiles of (sum of its steps) instead of the sum over steps of (max over
// tiles): with one kernel per step every kernel ends with a tail as long as its heaviest tile, and a tile's cost at one step
// says nothing about its cost at the next (measured correlation -0.2 .. -0.07; round 1: 315 -> 364 Mrays/s).
// CUBE = the exact-statistics build (egr_set_exact_stats): the tree bounds the reference's instance CUBES and every cube overlap
// is counted, so num_traversed_per_pixel is the reference's number (see forward_task.inc); images are the same.
#ifndef EGR_ARENA_CHUNK
#define EGR_ARENA_CHUNK 8 // hit-arena blocks a wave takes from the bump counter at a time (up to CHUNK - 1 blocks per resident wave stay unused: 29 k of the >= 469 k blocks of the reference's default capacity)
#endif
#ifndef EGR_FWD_WAVES
#define EGR_FWD_WAVES 4 // waves per SIMD the forward chain is built for (register budget 512 / EGR_FWD_WAVES)
#endif
template <bool GRADS, bool CUBE, int TEAM> __global__ void __launch_bounds__(EGR_WAVE * TEAM) __attribute__((amdgpu_waves_per_eu(EGR_FWD_WAVES, EGR_FWD_WAVES))) k_forward_chain(DeviceView v) {
    constexpr bool BATCH = false, OBJ = false;
    [[maybe_unused]] const ObjectQuery oq{};
    [[maybe_unused]] float *const oacc = nullptr;
#include "forward_chain.inc"
}
// The same chain for a batch of no-grad frames (egr_render_views): the frame is part of the task index, the primary rays read the frame's
// view record, and only the batch's last frame writes stats / random_seeds. Its own kernel, so that the launches of egr_raytrace keep theirs.
template <bool CUBE, int TEAM> __global__ void __launch_bounds__(EGR_WAVE * TEAM) __attribute__((amdgpu_waves_per_eu(EGR_FWD_WAVES, EGR_FWD_WAVES))) k_forward_batch(DeviceView v) {
    constexpr bool GRADS = false, BATCH = true, OBJ = false;
    [[maybe_unused]] const ObjectQuery oq{};
    [[maybe_unused]] float *const oacc = nullptr;
#include "forward_chain.inc"
}
// ... and for the views of a multi-view training launch (egr_train_views): one sample per view, hits recorded for the backward into the batch's own arena.
template <bool CUBE, int TEAM> __global__ void __launch_bounds__(EGR_WAVE * TEAM) __attribute__((amdgpu_waves_per_eu(EGR_FWD_WAVES, EGR_FWD_WAVES))) k_forward_batch_grads(DeviceView v) {
    constexpr bool GRADS = true, BATCH = true, OBJ = false;
    [[maybe_unused]] const ObjectQuery oq{};
    [[maybe_unused]] float *const oacc = nullptr;
#include "forward_chain.inc"
}
// ... and for egr_object_masks: the primary step of ONE view of the batch path with per-object coverage in place of the appearance (forward_task.inc: OBJ).
// Single-wave workgroups only, the product tree only. The coverage sums are [K][64] fp32 of DYNAMIC LDS behind the wave's WalkShared - K x 256 B, sized by
// the launch, so a query for four objects keeps the chain's sixteen waves per CU and one for thirty-two runs at what 160 KB hold.
#ifndef EGR_OBJ_WAVES
#define EGR_OBJ_WAVES EGR_FWD_WAVES // waves per SIMD k_forward_objects is built for (3: 168 VGPRs and no spill, but twelve waves per CU at any K - measured slower)
#endif
#ifndef EGR_OBJ_MIN_SUMS
#define EGR_OBJ_MIN_SUMS 1 // objects the LDS sums are sized for at least (32 = a fixed [32][64] array whatever K: the measurement of what sizing by K saves)
#endif
extern __shared__ float egr_object_sums[];
__global__ void __launch_bounds__(EGR_WAVE) __attribute__((amdgpu_waves_per_eu(EGR_OBJ_WAVES, EGR_OBJ_WAVES))) k_forward_objects(DeviceView v, ObjectQuery oq) {
    constexpr bool GRADS = false, BATCH = true, OBJ = true, CUBE = false;
    constexpr int TEAM = 1;
    float *const oacc = egr_object_sums;
#include "forward_chain.inc"
}
// The membership words of a query in record order: word of position p = bit j set iff row_bits[gid_of_pos[p]] has the j-th requested selection bit. One
// coalesced pass, so the chain's fetch is one load by the record index it already holds.
__global__ void __launch_bounds__(256) k_object_bits(DeviceView v, const uint32_t *__restrict__ row_bits, ObjectBitList bits, uint32_t num_bits, uint32_t *__restrict__ pos_bits) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= v.n) return;
    const uint32_t w = row_bits[v.gid_of_pos[p]];
    uint32_t out = 0u;
    for (uint32_t j = 0; j < num_bits; j++) out |= ((w >> bits.bit[j]) & 1u) << j;
    pos_bits[p] = out;
}
// k_batch_prologue + k_batch_chunk_begin for a query: the per-launch control words and fresh queues. metadata is not touched.
__global__ void k_objects_prologue(DeviceView v) {
    reset_launch_words(v, threadIdx.x);
    reset_chunk_words(v, threadIdx.x);
}

// ---------------------------------------------------------------------------------------------------------
// backward: walked newest (farthest) hit first  (backward_pass.cu:3-222)
// ---------------------------------------------------------------------------------------------------------
// Gradient pre-reduction (cdna guide, Guideline 12): the 64 primary rays of a tile composite the same few dozen Gaussians,
// so per-hit contributions are first summed in a per-wave LDS hash table (ds_add_f32, open addressing on the
// record index) and flushed once per tile: ~8x fewer global atomics than backward_pass.cu:210-220's 15/22 per hit.
#ifndef EGR_GT_SLOTS
#define EGR_GT_SLOTS 80 // slots of the primary step's LDS table (any count >= 64; multiply-shift hash). Since a full table is flushed and refilled
                        // (round 4) a smaller one is as good: 64 / 72 / 80 / 94 slots -> 3.02 / 3.05 / 3.01-3.03 / 3.11 ms backward chain
                        // dense-init (same box). Before that: 94 beat 64 (hits without a slot left as records of their own), 128 and 256 cost waves per CU
#endif
#define EGR_GT_COMPS 21
#define EGR_GT_STRIDE 21 // floats per table slot ([slot][component], odd stride: lanes on different slots fall on different LDS banks)
#define EGR_GT_EMPTY 0xFFFFFFFFu
// cell order of a gradient row (DeviceView::grad_rows; 21 of its 32 floats used), laid out by 64-B SEGMENT: the L2 retires atomic requests per 64-B segment,
// so every record falls into one. Segment 0 (cells 0-13) is what EVERY hit adds to - opacity, mean, rgb, weight and the six components of its symmetric local
// matrix Q (hit_geometry_fn) - and is the whole record of a BOUNCE hit; segment 1 (cells 16-22) holds what only a primary hit has. No hit writes a scale or
// rotation gradient: k_grad_gather applies the scale / rotation chain to the summed Q, once per gaussian.
enum : int { GC_OPA = 0, GC_MEAN = 1, GC_RGB = 4, GC_WEIGHT = 7, GC_Q = 8, GC_NORMAL = 16, GC_F0 = 19, GC_ROUGH = 22 };
// component order of a PRIMARY hit (the LDS table): components 0-13 are segment 0 cell for cell (Q: xx xy xz yy yz zz), components 14-20 go to segment 1
enum : int { PC_OPA = 0, PC_MEAN = 1, PC_RGB = 4, PC_WEIGHT = 7, PC_Q = 8, PC_NORMAL = 14, PC_F0 = 17, PC_ROUGH = 20 };
// the two records: (first row cell, components). A bounce hit is one REC0; a flushed table slot or a primary hit without a slot is one REC0 and one REC1.
#define EGR_REC0_CELL 0
#define EGR_REC0_COMPS 14
#define EGR_REC1_CELL 16
#define EGR_REC1_COMPS 7
static_assert(EGR_REC0_COMPS + EGR_REC1_COMPS == EGR_GT_COMPS && PC_NORMAL == EGR_REC0_COMPS && GC_NORMAL == EGR_REC1_CELL, "the table's components are the two records, in order");
#define EGR_ROW_STRIDE 32 // floats per gradient row: one 128-B line per gaussian
#define EGR_BWD_SYNC() wave_sync() // the backward chain's waves run independently (like the forward's): phases that exchange data through LDS within ONE wave need no more than program order

// SIXTEEN LANES PER RECORD add the N values of every lane with `ok` to the cells CELL .. CELL + N - 1 of its gaussian's gradient row - one 64-B atomic request per record, nothing returned, so the requests drain behind the wave's arithmetic
// (a lane adding its own N values issues N x 64 scattered 4-B requests per instruction row; the earlier record paths -
// per-block buckets + counting-sort reduce, per-wave record logs + an apply kernel - are measured in DESIGN.md 4 and gone).
// Wave-uniform call; `stage` = 64 x 4 float4.
template <int CELL, int N> EGR_DI void wide_add_wave(const DeviceView &v, bool ok, uint32_t pos, const float (&r)[N], float4 *stage) {
    static_assert(N >= 1 && N <= 15, "a record is its row index and up to 15 values: 16 lanes");
    static_assert(CELL >= 0 && CELL / 16 == (CELL + N - 1) / 16 && CELL + N <= EGR_ROW_STRIDE, "a record's cells lie in ONE 64-B segment of the row");
    const int lane = threadIdx.x & (EGR_WAVE - 1);
    const uint32_t cell = (uint32_t)CELL + (uint32_t)((lane & 15) - 1); // the row cell of this lane's component (lane & 15) - 1
    if (ok) {
        auto rv = [&](int i) { return i < N ? r[i < N ? i : 0] : 0.0f; };
        stage[4 * lane + 0] = make_float4(u2f(pos), rv(0), rv(1), rv(2));
        if (N > 3) stage[4 * lane + 1] = make_float4(rv(3), rv(4), rv(5), rv(6));
        if (N > 7) stage[4 * lane + 2] = make_float4(rv(7), rv(8), rv(9), rv(10));
        if (N > 11) stage[4 * lane + 3] = make_float4(rv(11), rv(12), rv(13), rv(14));
    }
    const unsigned long long okm = __ballot(ok);
    EGR_BWD_SYNC();
    const float *sf = reinterpret_cast<const float *>(stage);
#pragma unroll 4
    for (int pass = 0; pass < 16; pass++) {
        const int src = 4 * pass + (lane >> 4), c = lane & 15;
        if (((okm >> (4 * pass)) & 0xFull) == 0ull) continue; // wave-uniform: none of these four records exists
        const float x = sf[16 * src + c];
        const uint32_t p = f2u(sf[16 * src]);
        if (((okm >> src) & 1ull) && c != 0 && c <= N && x != 0.0f) atomicAdd(v.grad_rows + (size_t)p * EGR_ROW_STRIDE + cell, x); // (c > N: a stale stage word)
    }
    EGR_BWD_SYNC();
}

// Flush of the primary step's LDS table: every used slot leaves as two 16-lane records, one per segment of its row (components 0-13 and 14-20).
EGR_DI uint32_t grad_table_flush(const DeviceView &v, uint32_t *gt_keys, float *gt_vals, float4 *stage, int lane) {
    uint32_t sent = 0u; // records (two per used slot)
    EGR_BWD_SYNC();
    for (int s0 = 0; s0 < EGR_GT_SLOTS; s0 += EGR_WAVE) { // wave-uniform: wide_add_wave is a wave-level operation
        const int s = min(s0 + lane, EGR_GT_SLOTS - 1); // (a slot count that is no multiple of 64: the lanes beyond the table idle on its last slot)
        const bool in_table = s0 + lane < EGR_GT_SLOTS;
        const uint32_t pos = in_table ? gt_keys[s] : EGR_GT_EMPTY;
        const bool valid = pos != EGR_GT_EMPTY;
        if (in_table) gt_keys[s] = EGR_GT_EMPTY;
        float lo[EGR_REC0_COMPS], hi[EGR_REC1_COMPS];
#pragma unroll
        for (int c = 0; c < EGR_REC0_COMPS; c++) {
            lo[c] = valid ? gt_vals[s * EGR_GT_STRIDE + c] : 0.0f;
            if (valid) gt_vals[s * EGR_GT_STRIDE + c] = 0.0f; // (an unused slot holds zeros already)
        }
#pragma unroll
        for (int c = 0; c < EGR_REC1_COMPS; c++) {
            hi[c] = valid ? gt_vals[s * EGR_GT_STRIDE + EGR_REC0_COMPS + c] : 0.0f;
            if (valid) gt_vals[s * EGR_GT_STRIDE + EGR_REC0_COMPS + c] = 0.0f;
        }
        if (__ballot(valid) == 0ull) continue;
        wide_add_wave<EGR_REC0_CELL>(v, valid, pos, lo, stage);
        wide_add_wave<EGR_REC1_CELL>(v, valid, pos, hi, stage);
        sent += 2u * (uint32_t)__popcll(__ballot(valid));
    }
    EGR_BWD_SYNC();
    return sent;
}

// The 21 gradient components of the PRIMARY hits of one hit row (one per lane; `pos` = record index) on their way into the wave's LDS table
// (primary_table_add; it returns true for a lane whose contribution found no slot and has to leave as two records of its own). A row's sums need
// neither an order nor the table: the lanes of a row that hold the SAME gaussian are summed in registers, and one lane per gaussian - the leader -
// takes the sum to the table in a single pass.
//  (1) The table, keyed by record index, private to this wave. Every lane with a hit finds its gaussian's slot with plain reads (one CAS when it has
//      to create it: lanes with different keys can meet on one empty slot). LDS float atomics retire about ONE LANE PER CLOCK PER CU, shared by all
//      resident waves (22 ds_add_f32 per hit row made the table half of the backward chain in round 3), so a slot is updated with plain
//      ds_read / ds_write (conflict-free: odd slot stride) - by ONE lane.
//  (2) The lanes of a slot link up: each swaps its lane id into the slot's claim word and gets the lane that came before it (ds_wrxchg_rtn: one LDS
//      instruction for the whole row), the last one finds its own id there, leads, and empties the word again. Then pointer jumping: while any lane has
//      a predecessor, every lane pulls its predecessor's 21 components (ds_bpermute: independent pulls, no LDS memory) and adds them, and takes over
//      its predecessor's predecessor. A lane pulled from holds the sum of the list behind it, so after ceil(log2(largest group)) steps the leader holds
//      the group's sum - 3.3 steps per row on the dense-init cloud (55 active lanes, 17 gaussians per row: tools/primary_row_groups.py).
//      Until round 21 equal x / y neighbours were summed first (two DPP levels, primary_presum), every lane that was left (41 per row) came to the table,
//      and the lanes of a slot were served one per round through the claim word: 6.1 serialised read-modify-write rounds per row, counted on the GPU.
//      Also measured and not kept (profiles/HISTORY.md, profiles/r21/): the same tree behind a scalar loop that matches the lanes by record index
//      (readlane + ballot per distinct gaussian: 17 iterations per row, slower than the rounds), and the DPP levels in front of the list (no gain).
//  (3) A lane that finds no slot within 8 probes: the table is (as good as) full. A tile of the dense-init cloud composites more gaussians
//      (~ 100-130) than the table holds, and every hit of a gaussian without a slot used to leave the wave as two 64-B records of its own -
//      a resident gaussian costs two per TILE. The hits of a tile arrive far to near, layer by layer, so what a full table holds is mostly
//      done with: the wave empties it (two records per used slot, counted in `records`) and looks its hits up again.
// Wave-level; `want` = this lane holds a hit. `gx` of a leader ends as its group's sum (of any other lane: a partial sum nobody reads).
// `steps`, `leaders`: pointer-jumping steps and leaders of this row (wave-uniform; read by the EGR_TRAVERSAL_STATS build only).
EGR_DI bool primary_table_add(const DeviceView &v, const bool want, const uint32_t pos, float (&gx)[EGR_GT_COMPS], uint32_t *gt_keys, float *gt_vals, uint32_t *gt_claim, float4 *stage,
                              const int lane, uint32_t &records, uint32_t &steps, uint32_t &leaders) {
#pragma clang fp contract(off) // (a gx[c] that is a product stays a product: the add below is an add of the PULLED value)
    bool found = false;
    uint32_t slot = 0u;
    auto probe = [&]() {
        slot = ((((pos * 2654435761u) >> 16) * (uint32_t)EGR_GT_SLOTS) >> 16); // keyed by record index (multiply-shift: any slot count)
        found = false;
#pragma unroll 1
        for (int pr = 0; pr < (want ? 8 : 0); pr++) {
            uint32_t key = lds_peek(&gt_keys[slot]);
            if (key == EGR_GT_EMPTY) key = atomicCAS(&gt_keys[slot], EGR_GT_EMPTY, pos), key = key == EGR_GT_EMPTY ? pos : key; // (another lane of this row may have taken it meanwhile)
            if (key == pos) { found = true; break; }
            slot = slot + 1u == (uint32_t)EGR_GT_SLOTS ? 0u : slot + 1u;
        }
    };
    probe();
    if (__ballot(want && !found) != 0ull) {
        records += grad_table_flush(v, gt_keys, gt_vals, stage, lane);
        probe();
    }
    // (2) the lanes of a slot as a list: `prev` = the lane that came before this one, this lane itself: none
    uint32_t prev = (uint32_t)lane;
    if (found) {
        const uint32_t before = atomicExch(&gt_claim[slot], (uint32_t)lane);
        prev = before == EGR_GT_EMPTY ? (uint32_t)lane : before;
    }
    EGR_BWD_SYNC();
    const bool leader = found && lds_peek(&gt_claim[slot]) == (uint32_t)lane; // the last lane of its slot
    if (leader) lds_poke(&gt_claim[slot], EGR_GT_EMPTY); // (the word is empty between rows)
    steps = 0u, leaders = (uint32_t)__popcll(__ballot(leader));
    unsigned long long more = __ballot(prev != (uint32_t)lane);
#pragma unroll 1
    while (more != 0ull) { // wave-uniform: the pulls read every lane
        const bool take = prev != (uint32_t)lane;
        const int from = (int)(prev << 2);
        float o[EGR_GT_COMPS];
#pragma unroll
        for (int c = 0; c < EGR_GT_COMPS; c++) o[c] = __int_as_float(__builtin_amdgcn_ds_bpermute(from, __float_as_int(gx[c])));
        const uint32_t p2 = (uint32_t)__builtin_amdgcn_ds_bpermute(from, (int)prev);
#pragma unroll
        for (int c = 0; c < EGR_GT_COMPS; c++) { // add, then select (as `if (take) gx[c] += o[c]` the compiler keeps two copies of gx and moves between them: 0.2-0.4 ms)
            const float s = gx[c] + o[c];
            gx[c] = take ? s : gx[c];
        }
        prev = p2 == prev ? (uint32_t)lane : p2; // (the lane pulled from has none before it - it names itself -, or this lane pulled from itself: none)
        more = __ballot(prev != (uint32_t)lane);
        steps++;
    }
    if (leader) { // (1) the one pass: a slot is its leader's
        float *cell = gt_vals + slot * EGR_GT_STRIDE;
        float cur[EGR_GT_COMPS];
#pragma unroll
        for (int c = 0; c < EGR_GT_COMPS; c++) cur[c] = cell[c];
#pragma unroll
        for (int c = 0; c < EGR_GT_COMPS; c++) cell[c] = cur[c] + gx[c];
    }
    EGR_BWD_SYNC(); // (the next row's leader of this gaussian may be another lane)
    return want && !found; // (still no slot: the 21 components leave as two 16-lane records, like a flushed slot)
}

// ---- the scale / rotation chain (backward_pass.cu:170-205, activations.cu:66-73): d_scale and d_rot from L = (dl2w_0, dl2w_1, dl2w_2), the gradient with
// respect to the rows of the object->world matrix, and the gaussian's backward record (rows of M with exp(scale) in .w, raw quaternion). LINEAR in L with
// coefficients that belong to the gaussian alone: k_grad_gather applies it once per gaussian to the sum over all hits of a launch, primary and bounce
// (rebuilt from the summed Q of the gradient row). The one copy of the formula.
// Why double: d_rot is what the projection along q leaves of dL/dq, a small difference of large terms. Per hit the rounding errors of that
// difference average out over the hits of a gaussian; applied ONCE to the sum in fp32 the error of the one evaluation stays (measured: up to 2.8 x the
// fp32 reference's distance from the fp64 one, tests/test_hip_gradient_terms.py). One evaluation per gaussian is cheap enough to do in fp64.
struct ChainVec { double x, y, z; }; // (f3 is float only)
EGR_DI void scale_rot_chain(const float4 &M0, const float4 &M1, const float4 &M2, const float4 &qu, const float sigma, const float eps, const ChainVec &dl2w0, const ChainVec &dl2w1,
                            const ChainVec &dl2w2, double (&d_scale)[3], double (&d_rot)[4]) {
    using T = double;
    const T scaling_factor = sigma, eps_scale_grad = eps;
    const ChainVec scaling = {T(M0.w), T(M1.w), T(M2.w)}; // exp(scale), stored by k_instances
    const ChainVec den = {scaling.x * scaling_factor + eps_scale_grad, scaling.y * scaling_factor + eps_scale_grad, scaling.z * scaling_factor + eps_scale_grad};
    auto div3 = [&](const float4 &m) { return ChainVec{T(m.x) / den.x, T(m.y) / den.y, T(m.z) / den.z}; };
    const ChainVec rot_0 = div3(M0), rot_1 = div3(M1), rot_2 = div3(M2); // :178-180
    d_scale[0] = (dl2w0.x * rot_0.x + dl2w1.x * rot_1.x + dl2w2.x * rot_2.x) * scaling.x; // :181-182
    d_scale[1] = (dl2w0.y * rot_0.y + dl2w1.y * rot_1.y + dl2w2.y * rot_2.y) * scaling.y;
    d_scale[2] = (dl2w0.z * rot_0.z + dl2w1.z * rot_1.z + dl2w2.z * rot_2.z) * scaling.z;
    auto mul3 = [](const ChainVec &a, const ChainVec &b) { return ChainVec{a.x * b.x, a.y * b.y, a.z * b.z}; };
    const ChainVec dr0 = mul3(dl2w0, scaling), dr1 = mul3(dl2w1, scaling), dr2 = mul3(dl2w2, scaling); // :185-187
    const T qr = qu.x, qx = qu.y, qy = qu.z, qz = qu.w;
    const T qn = sqrt(qr * qr + qx * qx + qy * qy + qz * qz);
    const T r = qr / qn, x = qx / qn, y = qy / qn, z = qz / qn; // activations.cu:66-69
    const T dL_dr = T(2) * x * (dr2.y - dr1.z) + T(2) * y * (dr0.z - dr2.x) + T(2) * z * (dr1.x - dr0.y); // :194-205
    const T dL_dx = T(-4) * x * (dr1.y + dr2.z) + T(2) * y * (dr0.y + dr1.x) + T(2) * z * (dr0.z + dr2.x) + T(2) * r * (dr2.y - dr1.z);
    const T dL_dy = T(2) * x * (dr0.y + dr1.x) - T(4) * y * (dr0.x + dr2.z) + T(2) * z * (dr1.z + dr2.y) + T(2) * r * (dr0.z - dr2.x);
    const T dL_dz = T(2) * x * (dr0.z + dr2.x) + T(2) * y * (dr1.z + dr2.y) - T(4) * z * (dr0.x + dr1.y) + T(2) * r * (dr1.x - dr0.y);
    const T dd = dL_dr * qr + dL_dx * qx + dL_dy * qy + dL_dz * qz; // activations.cu:71-73
    const T qn3 = qn * qn * qn;
    const T inv3 = T(1) / qn3, inv1 = T(1) / qn;
    d_rot[0] = dd * -qr * inv3 + dL_dr * inv1, d_rot[1] = dd * -qx * inv3 + dL_dx * inv1;
    d_rot[2] = dd * -qy * inv3 + dL_dy * inv1, d_rot[3] = dd * -qz * inv3 + dL_dz * inv1;
}

// ---- the geometry half of B2 for one hit (backward_pass.cu:151-167) from the record position, the ray, the live (.., opacity, sigma) quarter and
// dL/dalpha. Independent of the other hits of the ray - the sequential half (suffix sums -> dL/dalpha) is the caller's.
// Every hit, primary or bounce, stops after d_mean and returns opacity, mean and six numbers (PC_* order = GC_* order: segment 0 of the row): the scale /
// rotation chain (:170-205) depends on the gaussian alone and is linear in dl2w, so it is applied once per gaussian to the launch's sum (k_grad_gather) -
// no fetch of the backward record (inst_m), no denominators, quotients or quaternion arithmetic per hit. What is summed is not dl2w itself but the LOCAL
// matrix Q = (-dL_dx_local * sigma) (x) local_hit, with dl2w_i = sum_k W_k,i * Q_k (W: the gaussian's world->object rows): dL_dx_local is a multiple of
// local_hit, so Q is symmetric - six components instead of nine - and a rounding error of the SUM is symmetric too. That matters: the rotation gradient is
// what is left of dl2w when its symmetric part cancels (nothing, for an isotropic gaussian), and a sum of the nine dl2w components carries an unsymmetric
// error of eps x sum |dl2w| into that difference (measured on a near-isotropic cloud, HIP's distance from the fp64 reference over the fp32 reference's, per
// loss term: 1.24-2.8 with dl2w summed and the chain in fp32; with Q and the chain in fp64 - scale_rot_chain - 0.33-0.95, as with the per-hit chain).
// With Q a bounce hit is 14 values (geometry 8 + 6, rgb 3, weight): still ONE 64-B record, because Q sits in segment 0 of the row.
template <class GX> EGR_DI void hit_geometry_fn(const DeviceView &v, const float exp_power, uint32_t pos, const float4 &a2, const f3 &ro, const f3 &rd, float dL_dalpha, GX &gx) {
    const float opacity = a2.z, scaling_factor = a2.w;
    // recompute the local hit exactly as the forward did
    const float4 W0 = v.inst_w[4 * pos], W1 = v.inst_w[4 * pos + 1], W2 = v.inst_w[4 * pos + 2];
    f3 lo, ld, dhat, u;
    float t_unused;
    bool behind_unused, outside_unused;
    candidate_geometry(W0, W1, W2, ro, rd, lo, ld, dhat, t_unused, u, behind_unused, outside_unused);
    const f3 local_hit = u * scaling_factor;
    const float sq_norm = dot(local_hit, local_hit);
    const float gaussval = egr_gaussian_sq(sq_norm, exp_power);

    float d_opacity = EGR_MAX_ALPHA * dL_dalpha * gaussval; // :151-152
    d_opacity = d_opacity * opacity * (1.0f - opacity);
    const float dL_dgaussval = EGR_MAX_ALPHA * dL_dalpha * opacity; // :155-158
    const float dL_dsq_norm = gaussval * pow_exp_m1(sq_norm, exp_power);
    const f3 dL_dx_local = (-local_hit * dL_dsq_norm) * dL_dgaussval;
    const f3 dL_dx_world = mk3(dot(mk3(W0.x, W1.x, W2.x), dL_dx_local), dot(mk3(W0.y, W1.y, W2.y), dL_dx_local),
                               dot(mk3(W0.z, W1.z, W2.z), dL_dx_local)) * scaling_factor; // :161-167
    const f3 d_mean = -dL_dx_world;
    gx[PC_OPA] = d_opacity, gx[PC_MEAN] = d_mean.x, gx[PC_MEAN + 1] = d_mean.y, gx[PC_MEAN + 2] = d_mean.z;
    const f3 ql = -dL_dx_local * scaling_factor;
    gx[PC_Q] = ql.x * local_hit.x, gx[PC_Q + 1] = ql.x * local_hit.y, gx[PC_Q + 2] = ql.x * local_hit.z;
    gx[PC_Q + 3] = ql.y * local_hit.y, gx[PC_Q + 4] = ql.y * local_hit.z, gx[PC_Q + 5] = ql.z * local_hit.z;
}

// One batch of 64 hits of a bounce step's queue (backward_chain.hpp: bounce_hits, pass 2), lane = hit: the geometry gradient from the hit's record index, the
// ray and dL/dalpha, the radiance part from the ray's dL/drgb, all 14 components (segment 0 of the row) out as one record. Queue, rays and radiance
// gradients are the LDS of the wave that OWNS the tile; `stage` is the executing wave's. Returns the records sent.
EGR_DI uint32_t bounce_batch(const DeviceView &v, const float exp_power, const uint4 *bitems, const float *bdl, const float *bray, uint32_t i0, uint32_t nitems, float4 *stage, int lane) {
    static_assert(PC_OPA == GC_OPA && PC_MEAN == GC_MEAN && PC_RGB == GC_RGB && PC_WEIGHT == GC_WEIGHT && PC_Q == GC_Q && GC_Q + 6 == EGR_REC0_COMPS, "components 0-13 of a hit are segment 0 of the row");
    const bool valid = i0 + (uint32_t)lane < nitems;
    uint32_t dpos = 0;
    float gx[EGR_REC0_COMPS];
#pragma unroll
    for (int c = 0; c < EGR_REC0_COMPS; c++) gx[c] = 0.0f;
    if (valid) {
        // (everything a hit needs beyond its gaussian's test record travels in the queue or sits in LDS: the fetches of this pass - live quarter
        // and W, one 64-B record - are ONE round trip; it used to re-read the arena row first and the ray from the state)
        const uint4 item = bitems[i0 + (uint32_t)lane];
        const uint32_t ray = item.x, pos = item.z;
        const float weight = u2f(item.w);
        const float4 a2 = v.inst_w[4 * pos + 3];
        const f3 iro = mk3(bray[ray], bray[EGR_WAVE + ray], bray[2 * EGR_WAVE + ray]), ird = mk3(bray[3 * EGR_WAVE + ray], bray[4 * EGR_WAVE + ray], bray[5 * EGR_WAVE + ray]);
        hit_geometry_fn(v, exp_power, pos, a2, iro, ird, u2f(item.y), gx);
        gx[GC_RGB] = bdl[ray] * weight, gx[GC_RGB + 1] = bdl[EGR_WAVE + ray] * weight, gx[GC_RGB + 2] = bdl[2 * EGR_WAVE + ray] * weight;
        gx[GC_WEIGHT] = weight;
        dpos = pos;
    }
    wide_add_wave<EGR_REC0_CELL>(v, valid, dpos, gx, stage);
    return (uint32_t)__popcll(__ballot(valid));
}

// Teams of the backward chain (under-filled ranks of a partition): per wave a ticket (epoch << 20 | batches << 10 | next batch) for the chunk of
// bounce hits it has queued, the number of items, and the batches done. No list order is at stake here - gradients are atomic adds.
#ifndef EGR_BWD_TEAM
#define EGR_BWD_TEAM 4 // waves per workgroup of the backward chain's team build
#endif
template <int TEAM> struct BwdTeamShared {
    uint32_t done;
    uint32_t ticket[TEAM], nitems[TEAM], finished[TEAM];
};

// The backward half of the fused per-tile chain (see k_forward_chain): a wave takes a tile's backward through all its steps - the
// primary step (21 gradient components per hit through the LDS table), then the bounce steps, last bounce first (14 components per
// hit, straight out as wide adds; in the team build their batches can be taken by team mates). Per-step code: backward_chain.hpp (backward_step).
#ifndef EGR_BWD_WAVES
#define EGR_BWD_WAVES 3
#endif
// Between the two chains of a grad launch: the order in which the backward chain takes this rank's tasks. The forward chain knows what a
// tile's backward will cost (its hit rows and hits), and a persistent-wave kernel ends with a tail as long as the tiles that START LATE and
// RUN LONG: per-task stamps of the whole image put the backward chain at 2807 us where a longest-first list schedule of the same task times
// needs 2289 us (dense-init; by this proxy 2323 us). One workgroup per queue chunk (wave_next_task: 8 chunks = compact image blocks, one
// per XCD) sorts ITS tasks by descending cost (stable counting sort over EGR_ORDER_BUCKETS = 16 cost classes) - a chunk's tiles stay on its XCD, only their order changes.
#ifndef EGR_ORDER_BUCKETS
#define EGR_ORDER_BUCKETS 16 // cost classes of the backward order
#endif
#ifndef EGR_ORDER_SHIFT
#define EGR_ORDER_SHIFT 7 // a class spans 2^7 = 128 units of cost (~ microseconds)
#endif
__global__ void __launch_bounds__(256) k_order_backward(DeviceView v) {
    // STABLE: inside a cost class the tiles keep the order of the chunk (a Z-curve over a compact image block: neighbours in time touch neighbouring records)
    __shared__ uint32_t cnt[EGR_ORDER_BUCKETS][256 + 1];
    const uint32_t chunk = ((v.num_tasks + 7u) / 8u + 3u) & ~3u, q = blockIdx.x;
    const uint32_t beg = q * chunk, end = min(beg + chunk, v.num_tasks);
    if (beg >= end) return;
    const uint32_t t = threadIdx.x, n = end - beg, per = (n + 255u) / 256u;
    const uint32_t i0 = min(t * per, n), i1 = min(i0 + per, n); // thread t owns the contiguous items [i0, i1) of the chunk
    auto bucket = [](uint32_t cost) { return (uint32_t)EGR_ORDER_BUCKETS - 1u - min(cost >> EGR_ORDER_SHIFT, (uint32_t)EGR_ORDER_BUCKETS - 1u); }; // (descending: costliest first)
    for (int b = 0; b < EGR_ORDER_BUCKETS; b++) cnt[b][t] = 0u;
    for (uint32_t i = i0; i < i1; i++) cnt[bucket(v.task_cost[beg + i])][t]++;
    __syncthreads();
    if (t < (uint32_t)EGR_ORDER_BUCKETS) { // exclusive scan over the threads, one cost class per thread
        uint32_t acc = 0u;
        for (int j = 0; j < 256; j++) {
            const uint32_t c = cnt[t][j];
            cnt[t][j] = acc, acc += c;
        }
        cnt[t][256] = acc;
    }
    __syncthreads();
    uint32_t start[EGR_ORDER_BUCKETS]; // where this thread's items of every class go
    uint32_t acc = 0u;
#pragma unroll
    for (int b = 0; b < EGR_ORDER_BUCKETS; b++) start[b] = acc + cnt[b][t], acc += cnt[b][256];
    for (uint32_t i = i0; i < i1; i++) {
        const uint32_t bk = bucket(v.task_cost[beg + i]);
        uint32_t at = 0u;
#pragma unroll
        for (int b = 0; b < EGR_ORDER_BUCKETS; b++)
            if ((uint32_t)b == bk) at = start[b]++;
        v.bwd_order[beg + at] = beg + i;
    }
}

// A team mate without tiles: take batches of the chunks its team mates have open (backward_chain.hpp: bounce_hits, the ticket) until all waves are through.
template <int TEAM> EGR_DI uint32_t bwd_team_help(const DeviceView &v, const float exp_power, BwdTeamShared<TEAM> &bteam, float (*gt_vals_all)[EGR_GT_STRIDE * EGR_GT_SLOTS],
                                                  float4 *stage, const int wv, const int lane) {
    uint32_t records = 0u;
    while (uniform_u32(lds_peek(&bteam.done)) < (uint32_t)TEAM) {
        bool any = false;
        for (int dlt = 1; dlt < TEAM; dlt++) {
            const int w = (wv + dlt) % TEAM;
            const uint32_t peek = uniform_u32(lds_peek(&bteam.ticket[w]));
            if ((peek & 0x3FFu) >= ((peek >> 10) & 0x3FFu)) continue; // nothing open there
            uint32_t tk = 0u;
            if (lane == 0) tk = atomicAdd(&bteam.ticket[w], 1u); // (epoch, batches and the batch taken come back in ONE word)
            tk = uniform_u32(tk);
            const uint32_t bi = tk & 0x3FFu, nbatch = (tk >> 10) & 0x3FFu;
            if (bi >= nbatch) continue;
            // the owner does not touch its queue, rays or radiance gradients before `finished` says that every batch of the chunk is done
            const uint32_t nitems = uniform_u32(lds_peek(&bteam.nitems[w]));
            const uint4 *bitems = reinterpret_cast<const uint4 *>(gt_vals_all[w]);
            records += bounce_batch(v, exp_power, bitems, gt_vals_all[w] + 16 * EGR_WAVE, gt_vals_all[w] + 19 * EGR_WAVE, bi * (uint32_t)EGR_WAVE, nitems, stage, lane);
            if (lane == 0) atomicAdd(&bteam.finished[w], 1u);
            any = true;
        }
        if (!any) __builtin_amdgcn_s_sleep(2);
    }
    return records;
}

#include "backward_chain.hpp"
template <int TEAM> __global__ void __launch_bounds__(EGR_WAVE * TEAM) __attribute__((amdgpu_waves_per_eu(EGR_BWD_WAVES, EGR_BWD_WAVES))) k_backward_chain(DeviceView v) {
    backward_chain<TEAM, false>(v);
}
// The same chain for the views of a multi-view training launch (egr_train_views). Its own kernel, so that the launches of egr_raytrace keep theirs.
template <int TEAM> __global__ void __launch_bounds__(EGR_WAVE * TEAM) __attribute__((amdgpu_waves_per_eu(EGR_BWD_WAVES, EGR_BWD_WAVES))) k_backward_batch(DeviceView v) {
    backward_chain<TEAM, true>(v);
}

// Last backward kernel: one thread per gaussian id adds its gradient row (a 128-B line at its record position) to the
// caller's gradient tensors - coalesced on the tensor side - and empties the row for the next launch.
// OVERWRITE (egr_set_grad_overwrite: the tensors are a per-launch buffer that is all-reduced over the ranks): the launch's sums are
// STORED, rows without a contribution store zeros - the caller neither clears the buffer nor pays the read half of a "+=".
// A row holds sums that are final (opacity, mean, rgb, weight, normal, f0, roughness) and, in its GC_Q cells, the summed local matrix Q of ALL the launch's
// hits (hit_geometry_fn): dl2w = W^T Q and the scale / rotation chain (scale_rot_chain) are applied to that sum here, once, with the records the hits
// read - nothing rewrites them between the chains and this kernel. Scale and rotation gradients exist only here, as locals.
// No cheap scatter kernel any more: the fp64 chain (seventeen quotients and a square root in double per hit gaussian) takes it from 38 to
// 98 VGPRs and from eight to four waves per SIMD; measured +0.015 ms on 0.095 ms at 1M gaussians (it still streams rows, records and nine tensors).
template <bool OVERWRITE> EGR_DI void grad_gather_row(const DeviceView &v, const uint32_t gid) {
    const size_t pos = v.pos_of_gid[gid];
    float4 *row = reinterpret_cast<float4 *>(v.grad_rows + pos * EGR_ROW_STRIDE);
    float x[EGR_ROW_STRIDE];
    uint32_t any = 0, any_l = 0;
#pragma unroll
    for (int q = 0; q < EGR_ROW_STRIDE / 4; q++) {
        const float4 r = row[q];
        x[4 * q] = r.x, x[4 * q + 1] = r.y, x[4 * q + 2] = r.z, x[4 * q + 3] = r.w;
        any |= (f2u(r.x) | f2u(r.y) | f2u(r.z) | f2u(r.w)) << 1; // ignore the sign bit: -0 is empty too
    }
    if (!OVERWRITE && any == 0) return;
    if (any != 0) {
#pragma unroll
        for (int q = 0; q < EGR_ROW_STRIDE / 4; q++) row[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int c = 0; c < 6; c++) any_l |= f2u(x[GC_Q + c]) << 1;
    float d_scale[3] = {0.f, 0.f, 0.f}, d_rot[4] = {0.f, 0.f, 0.f, 0.f}; // (a row without Q has none)
    if (any_l != 0) {
        const float4 *im = v.inst_m + 4 * (size_t)gid; // (the backward record is kept by id: coalesced)
        const float4 M0 = im[0], M1 = im[1], M2 = im[2], qu = im[3];
        const float4 W0 = v.inst_w[4 * pos], W1 = v.inst_w[4 * pos + 1], W2 = v.inst_w[4 * pos + 2];
        const float scaling_factor = v.inst_w[4 * pos + 3].w;
        const double q00 = x[GC_Q], q01 = x[GC_Q + 1], q02 = x[GC_Q + 2], q11 = x[GC_Q + 3], q12 = x[GC_Q + 4], q22 = x[GC_Q + 5];
        auto dl2w_of = [&](double w0, double w1, double w2) { return ChainVec{w0 * q00 + w1 * q01 + w2 * q02, w0 * q01 + w1 * q11 + w2 * q12, w0 * q02 + w1 * q12 + w2 * q22}; }; // dl2w_i = sum_k W_k,i Q_k
        double ds[3], dr[4];
        scale_rot_chain(M0, M1, M2, qu, scaling_factor, *v.cfg.eps_scale_grad, dl2w_of(W0.x, W1.x, W2.x), dl2w_of(W0.y, W1.y, W2.y), dl2w_of(W0.z, W1.z, W2.z), ds, dr);
#pragma unroll
        for (int a = 0; a < 3; a++) d_scale[a] = (float)ds[a];
#pragma unroll
        for (int a = 0; a < 4; a++) d_rot[a] = (float)dr[a];
    }
    const egr_gaussians &g = v.g;
    auto put = [](float *p, float val) {
        if (OVERWRITE) *p = val;
        else *p += val;
    };
    put(g.dL_dopacity + gid, x[GC_OPA]);
#pragma unroll
    for (int a = 0; a < 3; a++) {
        put(g.dL_dscale + 3 * gid + a, d_scale[a]), put(g.dL_dmean + 3 * gid + a, x[GC_MEAN + a]), put(g.dL_drgb + 3 * gid + a, x[GC_RGB + a]);
        put(g.dL_dnormal + 3 * gid + a, x[GC_NORMAL + a]), put(g.dL_df0 + 3 * gid + a, x[GC_F0 + a]);
    }
#pragma unroll
    for (int a = 0; a < 4; a++) put(g.dL_drotation + 4 * gid + a, d_rot[a]);
    put(g.dL_droughness + gid, x[GC_ROUGH]);
    put(g.total_weight + gid, x[GC_WEIGHT]);
}
// The import of one tensor for the 256 gaussians of a workgroup: `width` floats each, a contiguous run of both tensors - to += from, element by element, as
// float4s where the run is whole and both tensors are 16-byte aligned (a holder tensor starts 3n, 6n, ... floats into the flat gradient buffer).
EGR_DI void import_block_tensor(float *__restrict__ to, const float *from, const uint32_t block, const uint32_t n, const uint32_t width) {
    const size_t beg = (size_t)block * 256u * width, end = min(beg + (size_t)256u * width, (size_t)n * width);
    if (end - beg == (size_t)256u * width && ((reinterpret_cast<uintptr_t>(to) | reinterpret_cast<uintptr_t>(from)) & 15u) == 0) {
        float4 *to4 = reinterpret_cast<float4 *>(to + beg);
        const float4 *from4 = reinterpret_cast<const float4 *>(from + beg);
        for (uint32_t q = threadIdx.x; q < 64u * width; q += 256u) {
            float4 a = to4[q];
            const float4 b = from4[q];
            a.x += b.x, a.y += b.y, a.z += b.z, a.w += b.w;
            to4[q] = a;
        }
    } else {
        for (size_t j = beg + threadIdx.x; j < end; j += 256u) to[j] += from[j];
    }
}
// IMPORT (egr_raytrace_import; never with OVERWRITE): what this kernel leaves in the holder's gradient tensors - the accumulated value, also of a row without a
// contribution - is added to the caller's tensors `imp`: what a multi-tensor `caller.grad += holder.grad` after the launch computes, bit for bit. The
// workgroup's 256 gaussians are a contiguous run of every tensor, so once its threads have stored their sums (the barrier) the workgroup adds the runs as
// whole lines, like the multi-tensor kernel - but the holder's values are the ones it has just written: they come from the cache, and nothing is launched
// or read a second time. total_weight is not imported.
template <bool OVERWRITE, bool IMPORT> __global__ void __launch_bounds__(256) k_grad_gather(DeviceView v, EgrGradImport imp) {
    static_assert(!(OVERWRITE && IMPORT), "an importing launch adds");
    const uint32_t gid = blockIdx.x * 256 + threadIdx.x;
    if constexpr (!IMPORT) {
        if (gid >= v.n) return;
        grad_gather_row<OVERWRITE>(v, gid);
    } else {
        if (gid < v.n) grad_gather_row<false>(v, gid);
        __syncthreads(); // (workgroup scope: the stores above are visible to the loads below)
        const egr_gaussians &g = v.g;
        import_block_tensor(imp.dL_drgb, g.dL_drgb, blockIdx.x, v.n, 3), import_block_tensor(imp.dL_dnormal, g.dL_dnormal, blockIdx.x, v.n, 3);
        import_block_tensor(imp.dL_df0, g.dL_df0, blockIdx.x, v.n, 3), import_block_tensor(imp.dL_droughness, g.dL_droughness, blockIdx.x, v.n, 1);
        import_block_tensor(imp.dL_dopacity, g.dL_dopacity, blockIdx.x, v.n, 1), import_block_tensor(imp.dL_dscale, g.dL_dscale, blockIdx.x, v.n, 3);
        import_block_tensor(imp.dL_dmean, g.dL_dmean, blockIdx.x, v.n, 3), import_block_tensor(imp.dL_drotation, g.dL_drotation, blockIdx.x, v.n, 4);
    }
}

// ---------------------------------------------------------------------------------------------------------
// R6: output write / accumulation (shaders.cu:163-169, framebuffer.h:104-143); no-grad launches only
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(EGR_WAVE) k_finish(DeviceView v) {
    const int lane = threadIdx.x;
    const bool accumulate = *v.cfg.accumulate_samples != 0;
    const float cnt = accumulate ? (float)(*v.fb.accumulated_sample_count + 1) : 1.0f;
    const size_t P = v.num_pixels;
    for (uint32_t task = blockIdx.x; task < v.num_tasks; task += gridDim.x) {
        const TaskGeom tg = task_geom(v, task, lane);
        if (!tg.inside) continue;
        const StateRef S = state_of(v, task, lane);
        const uint32_t steps = f2u(S.ld(F_STEPS));
        f3 final = mk3(0, 0, 0);
        for (int s = 0; s < EGR_NSTEPS; s++) {
            const bool done = (uint32_t)s < steps;
            f3 rgb = done ? S.ld3(SF(s, S_RGB)) : mk3(0, 0, 0), n = done ? S.ld3(SF(s, S_NORMAL)) : mk3(0, 0, 0);
            f3 f0 = done ? S.ld3(SF(s, S_F0)) : mk3(0, 0, 0);
            float depth = done ? S.ld(SF(s, S_DEPTH)) : 0.0f, rough = done ? S.ld(SF(s, S_ROUGH)) : 0.0f;
            float T = done ? S.ld(SF(s, S_T)) : 1.0f, Ttot = done ? S.ld(SF(s, S_TTOT)) : 1.0f;
            f3 no = done ? S.ld3(SF(s, S_NEXT_O)) : mk3(0, 0, 0), nd = done ? S.ld3(SF(s, S_NEXT_D)) : mk3(0, 0, 0);
            const size_t q = tg.pixel_id + P * (size_t)s;
            if (accumulate) { // framebuffer.h:104-128
#define EGR_ACC3(buf, val) { float *a_ = v.fb.buf + 3 * q; a_[0] += val.x, a_[1] += val.y, a_[2] += val.z; val = div_s(mk3(a_[0], a_[1], a_[2]), cnt); }
#define EGR_ACC1(buf, val) { float *a_ = v.fb.buf + q; a_[0] += val; val = a_[0] / cnt; }
                EGR_ACC3(accumulated_rgb, rgb) EGR_ACC1(accumulated_transmittance, T) EGR_ACC1(accumulated_total_transmittance, Ttot)
                EGR_ACC1(accumulated_depth, depth) EGR_ACC3(accumulated_normal, n) EGR_ACC3(accumulated_f0, f0) EGR_ACC1(accumulated_roughness, rough)
#undef EGR_ACC3
#undef EGR_ACC1
            }
            final = final + rgb;
            float *o;
            o = v.fb.output_rgb + 3 * q, o[0] = rgb.x, o[1] = rgb.y, o[2] = rgb.z;
            o = v.fb.output_normal + 3 * q, o[0] = n.x, o[1] = n.y, o[2] = n.z;
            o = v.fb.output_f0 + 3 * q, o[0] = f0.x, o[1] = f0.y, o[2] = f0.z;
            o = v.fb.output_ray_origin + 3 * q, o[0] = no.x, o[1] = no.y, o[2] = no.z;
            o = v.fb.output_ray_direction + 3 * q, o[0] = nd.x, o[1] = nd.y, o[2] = nd.z;
            v.fb.output_depth[q] = depth, v.fb.output_roughness[q] = rough;
            v.fb.output_transmittance[q] = T, v.fb.output_total_transmittance[q] = Ttot;
        }
        float *o = v.fb.output_final + 3 * (size_t)tg.pixel_id;
        o[0] = final.x, o[1] = final.y, o[2] = final.z;
    }
}

// ---------------------------------------------------------------------------------------------------------
// batched no-grad render (egr_render_views): camera table, per-batch / per-chunk control, output write
// ---------------------------------------------------------------------------------------------------------
// One record per view from the dataset convention (k_set_camera's conversion, one thread per view): origin, rows of w2c, tanf(fov / 2) -
// what a single launch evaluates from the bound camera, the same operations - and after the last view the batch's znear / zfar, which the
// batch's DeviceView points cam.znear / cam.zfar at.
__global__ void k_batch_cameras(const float *__restrict__ R, const float *__restrict__ centre, const float *__restrict__ fov, uint32_t views, float znear, float zfar,
                                float *__restrict__ table) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == views) table[(size_t)views * EGR_BATCH_CAM_FLOATS] = znear, table[(size_t)views * EGR_BATCH_CAM_FLOATS + 1] = zfar;
    if (i >= views) return;
    float *rec = table + (size_t)i * EGR_BATCH_CAM_FLOATS;
    const float *r9 = R + 9 * (size_t)i;
    for (int t = 0; t < 9; t++) {
        const int r = t / 3, c = t % 3;
        rec[3 + 3 * c + r] = c == 0 ? r9[t] : -r9[t]; // w2c = transpose of the Blender c2w ((-R)[:, 0] *= -1)
    }
    for (int a = 0; a < 3; a++) rec[a] = centre[3 * (size_t)i + a];
    rec[12] = tanf(fov[i] / 2.0f);
    rec[13] = rec[14] = rec[15] = 0.0f;
}
// k_prologue for a batch: the per-launch control words, grads_enabled = grads (0: egr_render_views, 1: egr_train_views); total_num_calls stays as it is
// until k_batch_epilogue (the chunks derive every frame's seed from it).
__global__ void k_batch_prologue(DeviceView v, int grads) {
    reset_launch_words(v, threadIdx.x);
    if (threadIdx.x == 0) *v.meta.grads_enabled = grads ? 1 : 0;
}
// every chunk (the lists and hits of the previous chunk's tiles are done with: its backward ran before this chunk's forward)
__global__ void k_batch_chunk_begin(DeviceView v) { reset_chunk_words(v, threadIdx.x); }
__global__ void k_batch_epilogue(DeviceView v, uint32_t frames) {
    if (threadIdx.x == 0) {
        *v.meta.total_num_calls += (int32_t)frames; // metadata.h:30, once per frame
        count_lifetime(v, frames);
    }
}
struct BatchOutputs {
    float *final, *rgb, *depth, *normal, *f0, *roughness; // egr_view_batch's per-view buffers (NULL: not written)
};
// k_finish for a chunk of a batch: per pixel, the chunk's frames in order; a view's samples are summed in sample order (fp32, k_finish's
// EGR_ACC* operations) and its outputs written when its last sample arrives. A view that continues in the next chunk leaves its running
// sums in the carry buffer (at most one view spans a chunk boundary). S == 1: the values are written as they are (a non-accumulating launch).
__global__ void __launch_bounds__(EGR_WAVE) k_finish_batch(DeviceView v, BatchOutputs out, float *__restrict__ carry) {
    const int lane = threadIdx.x;
    const size_t P = v.num_pixels;
    const uint32_t S = v.batch_spv, B = v.batch_frames, sh = v.task_shift;
    const float cnt = (float)S;
    constexpr int NF = 11; // carried floats per step
    for (uint32_t task = blockIdx.x; task < v.num_tasks; task += gridDim.x) {
        const TaskGeom tg = task_geom(v, task, lane);
        if (!tg.inside) continue;
        float acc[EGR_NSTEPS][NF];
        if (v.batch_frame0 % S != 0) { // the chunk starts inside a view
#pragma unroll
            for (int s = 0; s < EGR_NSTEPS; s++)
#pragma unroll
                for (int k = 0; k < NF; k++) acc[s][k] = carry[(size_t)(s * NF + k) * P + tg.pixel_id];
        }
        for (uint32_t f = 0; f < B; f++) {
            const uint32_t frame = v.batch_frame0 + f, view = frame / S, sample = frame % S;
            if (sample == 0) {
#pragma unroll
                for (int s = 0; s < EGR_NSTEPS; s++)
#pragma unroll
                    for (int k = 0; k < NF; k++) acc[s][k] = 0.0f; // (reset_accumulators)
            }
            const StateRef St = state_of(v, (((task >> sh) * B + f) << sh) | (task & ((1u << sh) - 1u)), lane);
            const uint32_t steps = f2u(St.ld(F_STEPS));
            const bool last = sample == S - 1u;
            f3 final = mk3(0, 0, 0);
#pragma unroll
            for (int s = 0; s < EGR_NSTEPS; s++) {
                const bool done = (uint32_t)s < steps;
                f3 rgb = done ? St.ld3(SF(s, S_RGB)) : mk3(0, 0, 0), n = done ? St.ld3(SF(s, S_NORMAL)) : mk3(0, 0, 0);
                f3 f0 = done ? St.ld3(SF(s, S_F0)) : mk3(0, 0, 0);
                float depth = done ? St.ld(SF(s, S_DEPTH)) : 0.0f, rough = done ? St.ld(SF(s, S_ROUGH)) : 0.0f;
                if (S > 1u) { // framebuffer.h:104-128, as k_finish: running sum, then sum / count
                    float *a = acc[s];
                    a[0] += rgb.x, a[1] += rgb.y, a[2] += rgb.z, a[3] += depth, a[4] += n.x, a[5] += n.y, a[6] += n.z;
                    a[7] += f0.x, a[8] += f0.y, a[9] += f0.z, a[10] += rough;
                    if (!last) continue;
                    rgb = div_s(mk3(a[0], a[1], a[2]), cnt), depth = a[3] / cnt, n = div_s(mk3(a[4], a[5], a[6]), cnt);
                    f0 = div_s(mk3(a[7], a[8], a[9]), cnt), rough = a[10] / cnt;
                }
                final = final + rgb;
                const size_t q = tg.pixel_id + P * (size_t)s + 3 * P * (size_t)view; // [view][step][pixel]
                float *o;
                if (out.rgb) o = out.rgb + 3 * q, o[0] = rgb.x, o[1] = rgb.y, o[2] = rgb.z;
                if (out.normal) o = out.normal + 3 * q, o[0] = n.x, o[1] = n.y, o[2] = n.z;
                if (out.f0) o = out.f0 + 3 * q, o[0] = f0.x, o[1] = f0.y, o[2] = f0.z;
                if (out.depth) out.depth[q] = depth;
                if (out.roughness) out.roughness[q] = rough;
            }
            if (last) {
                float *o = out.final + 3 * ((size_t)tg.pixel_id + P * (size_t)view);
                o[0] = final.x, o[1] = final.y, o[2] = final.z;
            }
        }
        if ((v.batch_frame0 + B) % S != 0) { // the chunk ends inside a view: its sums continue in the next chunk
#pragma unroll
            for (int s = 0; s < EGR_NSTEPS; s++)
#pragma unroll
                for (int k = 0; k < NF; k++) carry[(size_t)(s * NF + k) * P + tg.pixel_id] = acc[s][k];
        }
    }
}

// Diagnostic export (egr_debug_get_step_hits): composited hits per pixel and bounce step of the last GRAD launch, from the ray state
// the backward chain reads (S_NHITS); steps a ray did not execute report 0. Pixels outside this rank's partition are not written.
__global__ void __launch_bounds__(EGR_WAVE) k_export_step_hits(DeviceView v, int32_t *__restrict__ out) {
    const int lane = threadIdx.x;
    for (uint32_t task = blockIdx.x; task < v.num_tasks; task += gridDim.x) {
        const TaskGeom tg = task_geom(v, task, lane);
        if (!tg.inside) continue;
        const StateRef S = state_of(v, task, lane);
        const uint32_t steps = f2u(S.ld(F_STEPS));
        for (int s = 0; s < EGR_NSTEPS; s++) out[(size_t)s * v.num_pixels + tg.pixel_id] = (uint32_t)s < steps ? (int32_t)f2u(S.ld(SF(s, S_NHITS))) : 0;
    }
}

// Diagnostic export (egr_debug_get_hit_sequence_hash): per pixel and step a hash of the ORDERED sequence of gaussian ids the last GRAD launch composited - the
// polynomial sum_i (id_i + 1) B^i mod 2^64 over the composite index i, evaluated back to front (Horner) along the step's arena chain, which is the order the
// backward walks; the CPU oracle evaluates the same sum front to back (oracle/egr_oracle.cpp: Outputs::hit_sequence_hash). Equal hashes = the same hits in the same order.
__global__ void __launch_bounds__(EGR_WAVE) k_export_hit_hash(DeviceView v, unsigned long long *__restrict__ out) {
    const int lane = threadIdx.x;
    constexpr unsigned long long B = 0x9E3779B97F4A7C15ull;
    for (uint32_t task = blockIdx.x; task < v.num_tasks; task += gridDim.x) {
        const TaskGeom tg = task_geom(v, task, lane);
        const StateRef S = state_of(v, task, lane);
        const uint32_t steps = tg.inside ? f2u(S.ld(F_STEPS)) : 0u;
        for (int s = 0; s < EGR_NSTEPS; s++) {
            uint32_t blk = v.task_last_block[(size_t)s * v.num_tasks + task];
            const uint32_t nhits = (tg.inside && (uint32_t)s < steps && blk != 0xFFFFFFFFu) ? f2u(S.ld(SF(s, S_NHITS))) : 0u;
            const uint32_t max_hits = wave_max_u32(nhits);
            unsigned long long h = 0ull;
            const uint32_t nblocks = (max_hits + EGR_HIT_BLOCK_ROWS - 1) / EGR_HIT_BLOCK_ROWS;
            for (uint32_t b = nblocks; b-- > 0 && blk != 0xFFFFFFFFu;) {
                const float4 *rows = v.hit_arena + (size_t)blk * (EGR_HIT_BLOCK_ROWS + 1) * EGR_WAVE;
                for (int row = EGR_HIT_BLOCK_ROWS - 1; row >= 0; row--)
                    if (b * EGR_HIT_BLOCK_ROWS + (uint32_t)row < nhits) h = h * B + (unsigned long long)v.gid_of_pos[f2u(rows[(size_t)(1 + row) * EGR_WAVE + lane].x)] + 1ull;
                blk = f2u(rows[0].x); // the block before this one (header row, lane 0's word)
            }
            if (tg.inside) out[(size_t)s * v.num_pixels + tg.pixel_id] = h;
        }
    }
}

// Camera upload: what gaussian_raytracer.py:94-100 does with ten tiny tensor kernels (R_blender = -R with column 0 negated back, three fill_ calls,
// set_pose's three copies) as ONE: R = the dataset's camera-to-world rotation (row-major 3x3), centre = camera_center, both device pointers.
__global__ void k_set_camera(egr_camera cam, const float *__restrict__ R, const float *__restrict__ centre, float fov, float znear, float zfar) {
    const int t = threadIdx.x;
    if (t < 9) {
        const int r = t / 3, c = t % 3;
        const float rb = c == 0 ? R[t] : -R[t]; // (-R)[:, 0] *= -1
        const_cast<float *>(cam.rotation_c2w)[t] = rb;
        const_cast<float *>(cam.rotation_w2c)[3 * c + r] = rb; // transpose
    }
    if (t < 3) const_cast<float *>(cam.origin)[t] = centre[t];
    if (t == 0) *const_cast<float *>(cam.vertical_fov_radians) = fov, *const_cast<float *>(cam.znear) = znear, *const_cast<float *>(cam.zfar) = zfar;
}
// ... with R and / or centre in HOST memory (a dataset's numpy pose): the twelve floats travel by value as a kernel argument - no upload, no wait, and the
// caller's arrays are free again when the launch call returns. A null device pointer = that part comes from `host`. The same stores as k_set_camera.
struct CameraPoseValues {
    float R[9], centre[3];
};
__global__ void k_set_camera_values(egr_camera cam, CameraPoseValues host, const float *__restrict__ R_dev, const float *__restrict__ centre_dev, float fov, float znear, float zfar) {
    const int t = threadIdx.x;
    if (t < 9) {
        const int r = t / 3, c = t % 3;
        const float x = R_dev ? R_dev[t] : host.R[t];
        const float rb = c == 0 ? x : -x;
        const_cast<float *>(cam.rotation_c2w)[t] = rb;
        const_cast<float *>(cam.rotation_w2c)[3 * c + r] = rb;
    }
    if (t < 3) const_cast<float *>(cam.origin)[t] = centre_dev ? centre_dev[t] : host.centre[t];
    if (t == 0) *const_cast<float *>(cam.vertical_fov_radians) = fov, *const_cast<float *>(cam.znear) = znear, *const_cast<float *>(cam.zfar) = zfar;
}

// Target upload (the caller's six `buf.copy_(val.moveaxis(0, -1))` of gaussian_raytracer.py:109-137 as ONE launch): CHW images -> the framebuffer's HWC
// target buffers, for the pixels of THIS rank's tiles only (a rank of an 8-way partition reads and writes an eighth of the 116 MB a whole
// 1080p frame moves); a missing image writes zeros, like the reference's `buf.zero_()`.
struct TargetImages {
    const float *chw[6]; // diffuse, specular, depth, normal, roughness, f0
};
__global__ void __launch_bounds__(EGR_WAVE) k_upload_targets(DeviceView v, TargetImages t) {
    const int lane = threadIdx.x;
    const size_t P = v.num_pixels;
    float *const dst[6] = {const_cast<float *>(v.fb.target_diffuse), const_cast<float *>(v.fb.target_specular), const_cast<float *>(v.fb.target_depth), const_cast<float *>(v.fb.target_normal), const_cast<float *>(v.fb.target_roughness), const_cast<float *>(v.fb.target_f0)}; // (the mirror of core/framebuffer.h declares the targets read-only for the launch)
    constexpr int ch[6] = {3, 3, 1, 3, 1, 3};
    for (uint32_t task = blockIdx.x; task < v.num_tasks; task += gridDim.x) {
        const TaskGeom tg = task_geom(v, task, lane);
        if (!tg.inside) continue;
#pragma unroll
        for (int b = 0; b < 6; b++)
#pragma unroll
            for (int c = 0; c < ch[b]; c++) dst[b][(size_t)ch[b] * tg.pixel_id + c] = t.chw[b] ? t.chw[b][(size_t)c * P + tg.pixel_id] : 0.0f;
    }
}

// The same for a tracer that owns the whole image (one rank): no tile geometry is needed, so the planes are read and the pixel-major
// buffers written 16 B per lane (four consecutive pixels per thread: 3 + 3 loads and stores for a colour buffer), 0.12 -> 0.05 ms per
// 1080p frame. Needs P % 4 == 0 and 16-B aligned planes (egr_upload_targets checks).
__global__ void __launch_bounds__(256) k_upload_targets_flat(DeviceView v, TargetImages t) {
    const size_t quads = v.num_pixels / 4, P = v.num_pixels;
    float *const dst[6] = {const_cast<float *>(v.fb.target_diffuse), const_cast<float *>(v.fb.target_specular), const_cast<float *>(v.fb.target_depth), const_cast<float *>(v.fb.target_normal), const_cast<float *>(v.fb.target_roughness), const_cast<float *>(v.fb.target_f0)};
    constexpr int ch[6] = {3, 3, 1, 3, 1, 3};
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (size_t)gridDim.x * blockDim.x) {
#pragma unroll
        for (int b = 0; b < 6; b++) {
            if (ch[b] == 1) {
                float4 a = t.chw[b] ? reinterpret_cast<const float4 *>(t.chw[b])[q] : make_float4(0.f, 0.f, 0.f, 0.f);
                reinterpret_cast<float4 *>(dst[b])[q] = a;
            } else {
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f), g = a, c = a;
                if (t.chw[b]) {
                    a = reinterpret_cast<const float4 *>(t.chw[b])[q];
                    g = reinterpret_cast<const float4 *>(t.chw[b] + P)[q];
                    c = reinterpret_cast<const float4 *>(t.chw[b] + 2 * P)[q];
                }
                float4 *o = reinterpret_cast<float4 *>(dst[b]) + 3 * q;
                o[0] = make_float4(a.x, g.x, c.x, a.y);
                o[1] = make_float4(g.y, c.y, a.z, g.z);
                o[2] = make_float4(c.z, a.w, g.w, c.w);
            }
        }
    }
}

__global__ void k_copy3(const float *__restrict__ src, float *__restrict__ dst, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// The chain kernels of the code object in the order it has always held them - the order of their first use, which this table now is (the compiler
// reports under profiles/ and the profiling tools list the kernels in it; where a launch names them has no say in it any more).
[[maybe_unused]] const void *const chain_kernel_order[] = {
#define K(...) reinterpret_cast<const void *>(&__VA_ARGS__)
    K(k_forward_chain<true, false, 1>), K(k_forward_chain<true, false, EGR_TEAM>), K(k_backward_chain<1>), K(k_forward_chain<true, true, EGR_TEAM>), K(k_forward_chain<false, true, EGR_TEAM>), K(k_forward_chain<false, false, EGR_TEAM>),
    K(k_forward_chain<true, true, 1>), K(k_forward_chain<false, true, 1>), K(k_forward_chain<false, false, 1>), K(k_backward_chain<EGR_BWD_TEAM>), K(k_grad_gather<true, false>), K(k_grad_gather<false, false>),
    K(k_forward_batch<true, EGR_TEAM>), K(k_forward_batch<false, EGR_TEAM>), K(k_forward_batch<true, 1>), K(k_forward_batch<false, 1>), K(k_forward_batch_grads<true, EGR_TEAM>), K(k_forward_batch_grads<false, EGR_TEAM>),
    K(k_forward_batch_grads<true, 1>), K(k_forward_batch_grads<false, 1>), K(k_backward_batch<EGR_BWD_TEAM>), K(k_backward_batch<1>), K(k_grad_gather<false, true>), K(k_forward_objects)
#undef K
};

} // namespace

uint32_t egr_num_tasks_for_rank(const egr_context *c) {
    uint32_t mtx = (c->width + EGR_MACRO_TILE - 1) / EGR_MACRO_TILE, mty = (c->height + EGR_MACRO_TILE - 1) / EGR_MACRO_TILE;
    const uint32_t M = mtx * mty, world = (uint32_t)c->world, rank = (uint32_t)c->rank;
    // every block of `world` consecutive Z-order positions holds each rank once; in the last, partial block b the positions j < rem go
    // to ranks (j + b) % world (see egr_build_task_order)
    const uint32_t full = M / world, rem = M % world;
    const uint32_t extra = ((rank + world - full % world) % world) < rem ? 1u : 0u;
    return 4u * (full + extra); // in 8x8 tiles; x 2 / x 4 with smaller tasks (egr_make_view)
}

// Which rank owns which macro tile ("tile k -> GPU k mod world after a Morton shuffle"): the macro tiles are sorted along a
// Z-curve over (mx, my); the tile at position i of that order belongs to rank (i + i / world) % world. Every run of `world` consecutive
// positions - a compact 2-D block of the image (eight ranks: 4 x 2 macro tiles) - holds each rank exactly once, and the rotation by the
// block index keeps a rank from sitting at the same place of every block (two ranks: a checkerboard, not columns). The plain
// `tile index % world` of rounds 1-3 gave every rank vertical 16-pixel column stripes whenever the number of tile columns was a
// multiple of the world size (120 at 1920 px: 2, 4, 8).
// Mirrors: parallel.tile_owner (Python), Oracle::set_partition (the CPU checker, oracle/egr_oracle.cpp); exported to C hosts as egr_tile_owner.
// Order of this rank's macro tiles: sort by (XCD chunk block, Z-curve inside the block). The 8 chunks that
// wave_next_task hands to the 8 XCD queues are equal slices of this order, so each is a compact image block.
static std::vector<std::pair<uint32_t, uint32_t>> egr_macro_tile_zorder(uint32_t mtx, uint32_t mty) { // (Z-curve key, macro tile) of the whole image, sorted
    auto part1by1 = [](uint32_t x) {
        x &= 0xFFFFu;
        x = (x | (x << 8)) & 0x00FF00FFu, x = (x | (x << 4)) & 0x0F0F0F0Fu, x = (x | (x << 2)) & 0x33333333u, x = (x | (x << 1)) & 0x55555555u;
        return x;
    };
    std::vector<std::pair<uint32_t, uint32_t>> zorder;
    zorder.reserve((size_t)mtx * mty);
    for (uint32_t m = 0; m < mtx * mty; m++) zorder.push_back({part1by1(m % mtx) | (part1by1(m / mtx) << 1), m});
    std::sort(zorder.begin(), zorder.end());
    return zorder;
}
extern "C" int egr_tile_owner(int width, int height, int world, int tile_index) {
    if (width <= 0 || height <= 0 || world < 1) return -1;
    const uint32_t mtx = ((uint32_t)width + EGR_MACRO_TILE - 1) / EGR_MACRO_TILE, mty = ((uint32_t)height + EGR_MACRO_TILE - 1) / EGR_MACRO_TILE;
    if (tile_index < 0 || (uint32_t)tile_index >= mtx * mty) return -1;
    const auto zorder = egr_macro_tile_zorder(mtx, mty);
    for (size_t i = 0; i < zorder.size(); i++)
        if (zorder[i].second == (uint32_t)tile_index) return (int)((i + i / (size_t)world) % (size_t)world);
    return -1;
}
void egr_build_task_order(egr_context *c) {
    for (const auto &o : c->task_orders)
        if (o.rank == c->rank && o.world == c->world) { // built before: kernels in flight keep reading the table they were launched with
            c->task_macro = o.table;
            return;
        }
    if (c->task_orders.size() >= 8) { // a caller cycling through many partitions: drop the cache (nothing may still read the tables)
        EGR_HIP(hipDeviceSynchronize());
        for (auto &o : c->task_orders) egr_dev_free(c, o.table);
        c->task_orders.clear();
    }
    const uint32_t mtx = (c->width + EGR_MACRO_TILE - 1) / EGR_MACRO_TILE, mty = (c->height + EGR_MACRO_TILE - 1) / EGR_MACRO_TILE;
    const std::vector<std::pair<uint32_t, uint32_t>> zorder = egr_macro_tile_zorder(mtx, mty);
    std::vector<std::pair<uint64_t, uint32_t>> keyed;
    for (size_t b = 0; b * (size_t)c->world < zorder.size(); b++) { // this rank's share: one tile of every block of `world` Z-order positions
        const size_t i = b * (size_t)c->world + (size_t)(((uint32_t)c->rank + (uint32_t)c->world - (uint32_t)(b % (size_t)c->world)) % (uint32_t)c->world);
        if (i >= zorder.size()) continue;
        const uint32_t m = zorder[i].second;
        const uint32_t mx = m % mtx, my = m / mtx;
        const uint32_t bx = std::min(3u, mx * 4u / mtx), by = std::min(1u, my * 2u / mty); // 4 x 2 blocks of the image
        const uint64_t key = ((uint64_t)(by * 4u + bx) << 32) | zorder[i].first;
        keyed.push_back({key, m});
    }
    std::sort(keyed.begin(), keyed.end());
    std::vector<uint32_t> order(std::max<size_t>(keyed.size(), 1), 0u);
    for (size_t i = 0; i < keyed.size(); i++) order[i] = keyed[i].second;
    uint32_t *table = nullptr;
    egr_dev_alloc(c, table, order.size());
    EGR_HIP(hipMemcpy(table, order.data(), order.size() * sizeof(uint32_t), hipMemcpyHostToDevice)); // pageable source: returns after the copy
    c->task_orders.push_back({c->rank, c->world, table});
    c->task_macro = table;
}

void egr_trace_free(egr_context *c) {
    egr_dev_free(c, c->batch_state), egr_dev_free(c, c->batch_carry), egr_dev_free(c, c->batch_cams);
    c->batch_alloc_frames = 0, c->batch_cams_cap = 0;
    egr_dev_free(c, c->object_bits), c->object_bits_cap = 0;
    egr_dev_free(c, c->train_arena), egr_dev_free(c, c->train_last_block), egr_dev_free(c, c->train_cost), egr_dev_free(c, c->train_order);
    c->train_alloc_frames = 0, c->train_blocks_cap = 0;
    for (auto &o : c->task_orders) egr_dev_free(c, o.table);
    c->task_orders.clear(), c->task_macro = nullptr;
    egr_dev_free(c, c->stack_spill), egr_dev_free(c, c->cand_keys), egr_dev_free(c, c->cand_vals), egr_dev_free(c, c->hit_arena), egr_dev_free(c, c->task_last_block), egr_dev_free(c, c->task_cost), egr_dev_free(c, c->bwd_order), egr_dev_free(c, c->state), egr_dev_free(c, c->control), egr_dev_free(c, c->queues), egr_dev_free(c, c->denoise_tmp), egr_dev_free(c, c->ext_keys), egr_dev_free(c, c->ext_vals);
    if (c->control_host) (void)hipHostFree(c->control_host);
    c->control_host = nullptr;
}

void egr_trace_alloc(egr_context *c) {
    uint32_t mtx = (c->width + EGR_MACRO_TILE - 1) / EGR_MACRO_TILE, mty = (c->height + EGR_MACRO_TILE - 1) / EGR_MACRO_TILE;
    c->num_tasks_total = 4u * mtx * mty;
    hipDeviceProp_t prop;
    EGR_HIP(hipGetDeviceProperties(&prop, c->device));
    int per_cu = 0; // the forward chain is built for four waves per SIMD (faster with more waves in flight even with spills)
    EGR_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (k_forward_chain<true, false, 1>), EGR_WAVE, 0));
    per_cu = std::max(1, std::min(32, per_cu));
    {
        int teams = 0; // the team build holds whole teams
        EGR_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&teams, (k_forward_chain<true, false, EGR_TEAM>), EGR_WAVE * EGR_TEAM, 0));
        c->team_waves_per_cu = std::max(1, teams) * EGR_TEAM;
    }
    if (getenv("EGR_DEBUG_OCCUPANCY")) {
        int bwd = 0;
        EGR_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&bwd, k_backward_chain<1>, EGR_WAVE, 0));
        fprintf(stderr, "[egr] resident waves per CU: forward chain %d, backward chain %d\n", per_cu, bwd);
    }
    if (const char *e = getenv("EGR_WAVES_PER_CU")) per_cu = std::max(1, std::min(per_cu, atoi(e))); // tuning knob
    uint32_t resident = (uint32_t)prop.multiProcessorCount * (uint32_t)per_cu;
    c->num_slots = std::max((uint32_t)EGR_TEAM, std::min(resident, (c->num_tasks_total + EGR_TEAM - 1u) / EGR_TEAM * EGR_TEAM)); // whole teams (the workgroups of the forward chain's team build)
    // forward budget: the reference's ppll_forward_size entries x 36 B, spent on (key 4 B + value 8 B) x 64 lanes x cap per slot
    // (the leaf pairs awaiting evaluation live in LDS since the pair walk: no queue in global memory)
    double fwd_bytes = (double)c->fwd_capacity * 36.0;
    uint64_t cap = (uint64_t)(fwd_bytes / ((double)c->num_slots * EGR_WAVE * 12.0)); // key 4 + value 8 bytes
    c->cand_cap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(cap, 64), 16384) & ~7u;
    egr_dev_alloc_raw(c, (void **)&c->cand_keys, (size_t)c->num_slots * c->cand_cap * EGR_WAVE * sizeof(float));
    egr_dev_alloc_raw(c, (void **)&c->cand_vals, (size_t)c->num_slots * c->cand_cap * EGR_WAVE * sizeof(float2));
    // extension blocks: 1/8 of the forward byte budget on top (12 B per entry), at least 64 blocks
    c->ext_blocks_cap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((uint64_t)(fwd_bytes / 8.0 / (12.0 * EGR_EXT_BLOCK)), 64), 65536);
    egr_dev_alloc_raw(c, (void **)&c->ext_keys, (size_t)c->ext_blocks_cap * EGR_EXT_BLOCK * sizeof(float));
    egr_dev_alloc_raw(c, (void **)&c->ext_vals, (size_t)c->ext_blocks_cap * EGR_EXT_BLOCK * sizeof(float2));
    egr_dev_alloc_raw(c, (void **)&c->stack_spill, (size_t)c->num_slots * EGR_GSTK * EGR_WAVE * sizeof(uint32_t));
    const double bwd_bytes = (double)c->bwd_capacity * 36.0; // the reference's ppll_backward_size entries x 36 B: all of it is arena
    uint64_t blocks = (uint64_t)(bwd_bytes / ((EGR_HIT_BLOCK_ROWS + 1) * EGR_WAVE * sizeof(float4)));
    c->hit_blocks_cap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(blocks, 64), 0x7FFFFFFFull);
    egr_dev_alloc_raw(c, (void **)&c->hit_arena, (size_t)c->hit_blocks_cap * (EGR_HIT_BLOCK_ROWS + 1) * EGR_WAVE * sizeof(float4));
    egr_dev_alloc_raw(c, (void **)&c->task_last_block, (size_t)EGR_NSTEPS * 4u * c->num_tasks_total * sizeof(uint32_t)); // (up to 16 tasks per macro tile)
    egr_dev_alloc_raw(c, (void **)&c->task_cost, (size_t)4u * c->num_tasks_total * sizeof(uint32_t));
    egr_dev_alloc_raw(c, (void **)&c->bwd_order, (size_t)4u * c->num_tasks_total * sizeof(uint32_t));
    if (const char *e = getenv("EGR_RAYS_PER_TASK")) c->rays_per_task = atoi(e);
    c->state_stride = c->num_tasks_total * EGR_WAVE;
    egr_dev_alloc_raw(c, (void **)&c->state, (size_t)F_TOTAL * c->state_stride * sizeof(float));
    EGR_HIP(hipMemset(c->state, 0, (size_t)F_TOTAL * c->state_stride * sizeof(float)));
    egr_dev_alloc_raw(c, (void **)&c->control, CW_COUNT * sizeof(uint32_t));
    EGR_HIP(hipMemset(c->control, 0, CW_COUNT * sizeof(uint32_t)));
    EGR_HIP(hipHostMalloc((void **)&c->control_host, CW_COUNT * sizeof(uint32_t)));
    egr_dev_alloc_raw(c, (void **)&c->queues, EGR_QUEUE_WORDS * sizeof(uint32_t));
    EGR_HIP(hipMemset(c->queues, 0, EGR_QUEUE_WORDS * sizeof(uint32_t)));
    egr_build_task_order(c);
}

// Team help of the next launch: on (default: a whole image's forward chain -6 % / -3 %, an under-filled rank's iteration -7 %), off, or - value -1 - on only for
// a rank of a partition with fewer than two 8x8 tiles per wave slot. With help the order of EXACT depth ties of bounce rays (0.1 % of the pixels of a 1080p frame
// hold one) varies from run to run, as it does upstream with the PPLL's insertion order; nothing else does (trace.hip: teams; forward_task.inc: total transmittance).
bool egr_team_help_on(const egr_context *c) {
    if (EGR_TEAM <= 1) return false;
    if (c->team_help >= 0) return c->team_help == 1;
    return c->world > 1 && egr_num_tasks_for_rank(c) < 2u * c->num_slots;
}

DeviceView egr_make_view(const egr_context *c) {
    DeviceView v{};
    v.width = c->width, v.height = c->height;
    v.tiles_x = (c->width + EGR_TILE - 1) / EGR_TILE, v.tiles_y = (c->height + EGR_TILE - 1) / EGR_TILE;
    v.num_pixels = (uint32_t)c->width * (uint32_t)c->height;
    v.n = c->g.count;
    v.num_nodes = c->num_wide;
    v.rank = c->rank, v.world = c->world;
    // Task size. 8x8 pixels unless the rank is under-filled: with fewer than two 8x8 tiles per resident wave (a rank of an 8-way
    // partition at 1080p) every tile starts at once and the launch lasts as long as its heaviest tile - 8x4-pixel tasks halve the
    // tiles (rank 0 of an emulated 8-way partition: 5.04 -> 4.16 ms dense-init, 3.95 -> 3.71 ms trained-like; 4x4 tasks: 4.12 / 4.12 ms,
    // the per-ray phases then run at a quarter of the lanes). A ray's candidate LIST ORDER depends on the task shape
    // (pair walk), so exactly tied depths may composite in another order than with 8x8 tasks (documented deviation (a)).
    const uint32_t tiles = egr_num_tasks_for_rank(c);
    uint32_t rpt = c->rays_per_task == 16 || c->rays_per_task == 32 || c->rays_per_task == 64 ? (uint32_t)c->rays_per_task
                   : (c->world > 1 && tiles < 2u * c->num_slots && !egr_team_help_on(c) ? 32u : 64u); // (with team help the heavy tile's walk is shared anyway, and whole 8x8 tiles keep all lanes busy in the per-ray phases: 3.08-3.12 against 3.17-3.21 ms trained-like, 3.50-3.55 against 3.48-3.51 ms dense-init per iteration of rank 0 of 8)
    v.rays_per_task = rpt, v.task_shift = rpt == 64u ? 2u : rpt == 32u ? 3u : 4u;
    v.num_tasks = tiles << (v.task_shift - 2u);
    v.queues = c->queues;
    v.task_macro = c->task_macro;
    // (help changes the ORDER in which a ray's candidates enter its list, never the set; egr_team_help_on)
    v.team_help = egr_team_help_on(c) ? 1 : 0;
    v.g = c->g, v.cfg = c->cfg, v.cam = c->cam, v.fb = c->fb, v.meta = c->meta, v.stats = c->stats;
    v.wnodes = c->wnodes, v.stack_spill = c->stack_spill, v.gid_of_pos = c->vals_out, v.pos_of_gid = c->pos_of_gid, v.frame = c->frame, v.out_of_frame = c->out_of_frame, v.inst_w = c->inst_w, v.inst_m = c->inst_m, v.grad_rows = c->grad_rows, v.app = c->app, v.bsph = c->bsph;
    v.cand_keys = c->cand_keys, v.cand_vals = c->cand_vals, v.cand_cap = c->cand_cap, v.num_slots = c->num_slots;
    v.ext_keys = c->ext_keys, v.ext_vals = c->ext_vals, v.ext_blocks_cap = c->ext_blocks_cap;
    v.hit_arena = c->hit_arena, v.hit_blocks_cap = c->hit_blocks_cap, v.task_last_block = c->task_last_block, v.task_cost = c->task_cost, v.bwd_order = c->bwd_order;
    v.state = c->state, v.state_stride = c->state_stride, v.control = c->control;
    v.cube_mode = c->exact_stats ? 1 : 0;
    v.pixel_mask = c->pixel_mask;
    v.grad_overwrite = (c->grad_overwrite && !c->delta_pending) ? 1 : 0;
    // (a single grad launch reads the framebuffer's pixel-major targets unless its caller hands it planes: egr_trace_launch)
    const float *const fbt[6] = {c->fb.target_diffuse, c->fb.target_specular, c->fb.target_depth, c->fb.target_normal, c->fb.target_roughness, c->fb.target_f0};
    for (int k = 0; k < 6; k++) v.batch_targets[k] = fbt[k];
    v.target_planes = 0u;
    return v;
}

// ---------------------------------------------------------------------------------------------------------
// the steps of a launch. egr_trace_launch, egr_render_views_launch and egr_train_views_launch below are sequences of them.
// ---------------------------------------------------------------------------------------------------------
namespace {

struct BatchCameras { // the camera arrays of an egr_view_batch / egr_train_batch
    const float *rotation_c2w_dataset, *camera_center, *vertical_fov_radians;
    uint32_t views;
    float znear, zfar;
};
template <class B> BatchCameras batch_cameras_of(const B *b) { return {b->rotation_c2w_dataset, b->camera_center, b->vertical_fov_radians, b->num_views, b->znear, b->zfar}; }

// The view of a batch of `views` x `spv` frames: ray state of a chunk of frames, the camera table with the batch's znear / zfar behind its last record.
DeviceView batch_view(const egr_context *c, uint32_t views, uint32_t spv) {
    DeviceView v = egr_make_view(c);
    v.state = c->batch_state, v.state_stride = c->state_stride * c->batch_alloc_frames;
    v.batch_cams = c->batch_cams, v.batch_spv = spv, v.batch_last_frame = views * spv - 1u;
    v.cam.znear = c->batch_cams + (size_t)views * EGR_BATCH_CAM_FLOATS, v.cam.zfar = v.cam.znear + 1;
    return v;
}

// The per-launch work in front of the chains: control words, stats reset, live records. `cams`: a batch (its camera table is written first, and
// total_num_calls waits for the batch's epilogue); NULL: a single launch.
void launch_begin(egr_context *c, const DeviceView &v, bool grads, bool live_fresh, const BatchCameras *cams, hipStream_t s) {
    egr_stamp_begin(c, "prologue+live", s);
    if (cams) {
        hipLaunchKernelGGL(k_batch_cameras, dim3((cams->views + 64u) / 64u), dim3(64), 0, s, cams->rotation_c2w_dataset, cams->camera_center, cams->vertical_fov_radians, cams->views, cams->znear, cams->zfar, c->batch_cams);
        hipLaunchKernelGGL(k_batch_prologue, dim3(1), dim3(64), 0, s, v, grads ? 1 : 0);
    } else {
        hipLaunchKernelGGL(k_prologue, dim3(1), dim3(64), 0, s, v, grads ? 1 : 0);
    }
    // stats.h:25-28. A launch whose tasks cover the whole image stores both counts of EVERY pixel at step 0 (forward_task.inc: `active` is `inside` there; a batch:
    // in its last frame, which always runs), so clearing them first is a pass over 8 B per pixel for nothing. A rank of a partition and a masked launch leave
    // pixels out, a rank without tasks all of them: those clear as ever.
    const bool stores_every_pixel = c->world == 1 && c->pixel_mask == nullptr && v.num_tasks != 0;
    if (!stores_every_pixel) {
        EGR_HIP(hipMemsetAsync(c->stats.num_accumulated_per_pixel, 0, sizeof(int32_t) * v.num_pixels, s));
        EGR_HIP(hipMemsetAsync(c->stats.num_traversed_per_pixel, 0, sizeof(int32_t) * v.num_pixels, s));
    }
    // (skipped when the egr_update_bvh_ex(EGR_UPDATE_FUSE_LIVE) just before this launch wrote the same records from the same parameters)
    if (v.n && !live_fresh) hipLaunchKernelGGL(k_live, dim3((v.n + 255) / 256), dim3(256), 0, s, v, grads ? 1 : 0);
    egr_stamp_end(c, s);
}

// One wave slot per task, at most num_slots: the persistent waves of either chain.
uint32_t chain_slots(const egr_context *c, uint32_t tasks) { return std::max(1u, std::min(c->num_slots, tasks)); }

// The forward chain over `tasks` tasks (a batch: tasks x the chunk's frames).
enum class ForwardKernel { single, single_grads, batch, batch_grads };
void launch_forward_chain(egr_context *c, const DeviceView &v, uint32_t tasks, ForwardKernel kernel, hipStream_t s) {
    const uint32_t slots = chain_slots(c, tasks);
    egr_stamp_begin(c, "forward_chain", s);
    auto launch = [&](auto team_tag, auto cube_tag) {
        constexpr int T = decltype(team_tag)::value;
        constexpr bool CUBE = decltype(cube_tag)::value;
        const dim3 grid((slots + T - 1u) / T), block(EGR_WAVE * T); // (num_slots is a multiple of EGR_TEAM: every wave of a team has its scratch)
        switch (kernel) {
        case ForwardKernel::single: hipLaunchKernelGGL((k_forward_chain<false, CUBE, T>), grid, block, 0, s, v); break;
        case ForwardKernel::single_grads: hipLaunchKernelGGL((k_forward_chain<true, CUBE, T>), grid, block, 0, s, v); break;
        case ForwardKernel::batch: hipLaunchKernelGGL((k_forward_batch<CUBE, T>), grid, block, 0, s, v); break;
        case ForwardKernel::batch_grads: hipLaunchKernelGGL((k_forward_batch_grads<CUBE, T>), grid, block, 0, s, v); break;
        }
    };
    auto launch_team = [&](auto team_tag) {
        if (v.cube_mode) launch(team_tag, std::true_type{});
        else launch(team_tag, std::false_type{});
    };
    // (the chain exists as single-wave workgroups and as teams of EGR_TEAM waves: launches with egr_set_team_help(1) take the teams)
    if (v.team_help) launch_team(std::integral_constant<int, EGR_TEAM>{});
    else launch_team(std::integral_constant<int, 1>{});
    egr_stamp_end(c, s);
}

// The backward order and the backward chain over the same `tasks` tasks the forward chain just ran. `batch`: the frame is part of the task index.
void launch_backward_chain(egr_context *c, const DeviceView &v, uint32_t tasks, bool batch, hipStream_t s) {
    const uint32_t slots = chain_slots(c, tasks);
    DeviceView ov = v; // k_order_backward sorts every queue chunk of the whole task range, the chunks the backward's wave_next_task hands out
    ov.num_tasks = tasks;
    hipLaunchKernelGGL(k_order_backward, dim3(8), dim3(256), 0, s, ov);
    egr_stamp_begin(c, "backward_chain", s);
    // (under-filled ranks: the backward chain as teams whose waves without tiles take batches of their mates' bounce hits - gradients are
    // atomic adds, so no result depends on who sends them; a whole image keeps single-wave workgroups: a team's LDS is only released with its last wave)
    // (egr_set_team_help(1) takes the teams of both chains: tests/test_hip_parity.py)
    const bool teams = v.team_help == 1 || (c->world > 1 && (uint64_t)(tasks >> (v.task_shift - 2u)) < 2ull * c->num_slots);
    const dim3 grid(teams ? (slots + EGR_BWD_TEAM - 1u) / EGR_BWD_TEAM : slots), block(teams ? EGR_WAVE * EGR_BWD_TEAM : EGR_WAVE);
    if (batch) {
        if (teams) hipLaunchKernelGGL(k_backward_batch<EGR_BWD_TEAM>, grid, block, 0, s, v);
        else hipLaunchKernelGGL(k_backward_batch<1>, grid, block, 0, s, v);
    } else {
        if (teams) hipLaunchKernelGGL(k_backward_chain<EGR_BWD_TEAM>, grid, block, 0, s, v);
        else hipLaunchKernelGGL(k_backward_chain<1>, grid, block, 0, s, v);
    }
    egr_stamp_end(c, s);
}

// The last step of a grad launch: the gradient rows to the caller's tensors.
void launch_grad_gather(egr_context *c, const DeviceView &v, const EgrGradImport *imp, hipStream_t s) {
    if (!(v.n && (v.num_tasks || c->grad_overwrite || imp))) return; // (a rank without tiles still owes its per-launch buffer a row of zeros, an importing caller what the holder has)
    egr_stamp_begin(c, "backward_grad_gather", s);
    // (per-launch buffer: the FIRST grad launch after the caller consumed the buffer stores, any further one before the next
    // egr_grad_delta_consumed adds - two launches before a fold never drop the first one's gradients)
    // (egr_raytrace_import refuses a context with a per-launch buffer: an importing launch always adds)
    if (imp) hipLaunchKernelGGL((k_grad_gather<false, true>), dim3((v.n + 255u) / 256u), dim3(256), 0, s, v, *imp);
    else if (v.grad_overwrite) hipLaunchKernelGGL((k_grad_gather<true, false>), dim3((v.n + 255u) / 256u), dim3(256), 0, s, v, EgrGradImport{});
    else hipLaunchKernelGGL((k_grad_gather<false, false>), dim3((v.n + 255u) / 256u), dim3(256), 0, s, v, EgrGradImport{});
    egr_stamp_end(c, s);
    if (c->grad_overwrite) c->delta_pending = true;
}

// Diagnostic exports: one zeroed device buffer of EGR_NSTEPS x pixels elements of type T, filled by KERNEL, copied to the host.
template <class T, void (*KERNEL)(DeviceView, T *)> void export_per_step(egr_context *c, void *host_out, hipStream_t s) {
    DeviceView v = egr_make_view(c);
    const size_t bytes = (size_t)EGR_NSTEPS * v.num_pixels * sizeof(T);
    struct DevBuf { // freed on every way out (an EGR_HIP below may throw)
        T *p = nullptr;
        ~DevBuf() { if (p) (void)hipFree(p); }
    } dev;
    EGR_HIP(hipMalloc((void **)&dev.p, bytes));
    EGR_HIP(hipMemsetAsync(dev.p, 0, bytes, s));
    if (v.num_tasks) hipLaunchKernelGGL(KERNEL, dim3(std::min(v.num_tasks, 65535u)), dim3(EGR_WAVE), 0, s, v, dev.p);
    EGR_HIP(hipMemcpyAsync(host_out, dev.p, bytes, hipMemcpyDeviceToHost, s));
    EGR_HIP(hipStreamSynchronize(s));
}

} // namespace

void egr_trace_launch(egr_context *c, bool grads, bool live_fresh, hipStream_t s, const EgrGradImport *import_into, const EgrTargetPlanes *targets) {
    DeviceView v = egr_make_view(c);
    if (targets) { // the backward reads the caller's channel-major images where they are: no upload, the framebuffer's target_* buffers are not touched
        for (int k = 0; k < 6; k++) v.batch_targets[k] = targets->chw[k];
        v.target_planes = 1u;
    }
    launch_begin(c, v, grads, live_fresh, nullptr, s);
    if (v.num_tasks) {
        launch_forward_chain(c, v, v.num_tasks, grads ? ForwardKernel::single_grads : ForwardKernel::single, s);
        if (grads) {
            launch_backward_chain(c, v, v.num_tasks, false, s);
        } else {
            egr_stamp_begin(c, "write_outputs", s);
            hipLaunchKernelGGL(k_finish, dim3(std::max(1u, std::min(v.num_tasks, 65535u))), dim3(EGR_WAVE), 0, s, v);
            egr_stamp_end(c, s);
        }
    }
    if (grads) launch_grad_gather(c, v, import_into, s);
    hipLaunchKernelGGL(k_epilogue, dim3(1), dim3(64), 0, s, v, grads ? 1 : 0);
}

// The buffers every batch needs: the ray state of B frames and the camera records of V views (allocated by the first batch call; they grow with a
// larger chunk / view count).
static void egr_batch_reserve(egr_context *c, uint32_t B, uint32_t V) {
    if (c->batch_alloc_frames < B || c->batch_cams_cap < V) EGR_HIP(hipDeviceSynchronize()); // (kernels in flight may still read the buffers replaced below)
    if (c->batch_alloc_frames < B) {
        egr_dev_free(c, c->batch_state);
        c->batch_alloc_frames = 0;
        egr_dev_alloc_raw(c, (void **)&c->batch_state, (size_t)F_TOTAL * B * c->state_stride * sizeof(float));
        c->batch_alloc_frames = B;
    }
    if (c->batch_cams_cap < V) {
        egr_dev_free(c, c->batch_cams);
        c->batch_cams_cap = 0;
        egr_dev_alloc(c, c->batch_cams, (size_t)(V + 1) * EGR_BATCH_CAM_FLOATS);
        c->batch_cams_cap = V;
    }
}

// egr_render_views: V x S frames in chunks of B = min(V x S, batch_frames) frames, in frame order. Each chunk is one forward chain over
// (this rank's tasks) x B and one k_finish_batch; the per-launch work of a single frame - prologue, stats reset, k_live, epilogue - runs
// once per batch.
void egr_render_views_launch(egr_context *c, const egr_view_batch *b, bool live_fresh, hipStream_t s) {
    const uint32_t V = b->num_views, F = b->num_views * b->samples_per_view;
    const uint32_t B = std::min(F, std::max(1u, c->batch_frames));
    egr_batch_reserve(c, B, V);
    if (!c->batch_carry) egr_dev_alloc(c, c->batch_carry, (size_t)EGR_BATCH_CARRY_FLOATS * c->width * c->height);
    DeviceView v = batch_view(c, V, b->samples_per_view);
    const BatchOutputs out{b->final, b->rgb, b->depth, b->normal, b->f0, b->roughness};
    const BatchCameras cams = batch_cameras_of(b);
    launch_begin(c, v, false, live_fresh, &cams, s);
    for (uint32_t f0 = 0; f0 < F && v.num_tasks; f0 += B) {
        v.batch_frame0 = f0, v.batch_frames = std::min(B, F - f0);
        hipLaunchKernelGGL(k_batch_chunk_begin, dim3(1), dim3(64), 0, s, v);
        launch_forward_chain(c, v, v.num_tasks * v.batch_frames, ForwardKernel::batch, s);
        egr_stamp_begin(c, "write_outputs", s);
        hipLaunchKernelGGL(k_finish_batch, dim3(std::max(1u, std::min(v.num_tasks, 65535u))), dim3(EGR_WAVE), 0, s, v, out, c->batch_carry);
        egr_stamp_end(c, s);
    }
    hipLaunchKernelGGL(k_batch_epilogue, dim3(1), dim3(64), 0, s, v, F);
}

// egr_train_views: V views (one sample each) in chunks of B = min(V, batch_frames) frames. Per chunk: the forward chain over (this rank's tasks) x B, which
// records every frame's hits into the batch arena, k_order_backward over the same (tasks x frames), and the backward chain over them - all three with the
// frame in the task index. Prologue, stats reset, k_live, k_grad_gather and the epilogue run once per call, so the chunks' gradients meet in the gradient
// rows and leave them in ONE gather (the whole batch is one grad launch for the per-launch buffer).
void egr_train_views_launch(egr_context *c, const egr_train_batch *b, bool live_fresh, hipStream_t s, const EgrGradImport *import_into) {
    const uint32_t V = b->num_views;
    const uint32_t B = std::min(V, std::max(1u, c->batch_frames));
    egr_batch_reserve(c, B, V);
    if (c->train_alloc_frames < B) { // hit arena (B x the single launch's) and per-task tables of a chunk of B frames
        EGR_HIP(hipDeviceSynchronize());
        egr_dev_free(c, c->train_arena), egr_dev_free(c, c->train_last_block), egr_dev_free(c, c->train_cost), egr_dev_free(c, c->train_order);
        c->train_alloc_frames = 0, c->train_blocks_cap = 0;
        const uint32_t cap = (uint32_t)std::min<uint64_t>((uint64_t)c->hit_blocks_cap * B, 0x7FFFFFFFull);
        egr_dev_alloc_raw(c, (void **)&c->train_arena, (size_t)cap * (EGR_HIT_BLOCK_ROWS + 1) * EGR_WAVE * sizeof(float4));
        const size_t tasks = (size_t)4u * c->num_tasks_total * B; // (up to 16 tasks per macro tile, as the single launch's tables)
        egr_dev_alloc(c, c->train_last_block, (size_t)EGR_NSTEPS * tasks);
        egr_dev_alloc(c, c->train_cost, tasks);
        egr_dev_alloc(c, c->train_order, tasks);
        c->train_alloc_frames = B, c->train_blocks_cap = cap;
    }
    DeviceView v = batch_view(c, V, 1u);
    v.hit_arena = c->train_arena, v.hit_blocks_cap = c->train_blocks_cap, v.task_last_block = c->train_last_block, v.task_cost = c->train_cost, v.bwd_order = c->train_order;
    const float *const tgt[6] = {b->target_diffuse, b->target_specular, b->target_depth, b->target_normal, b->target_roughness, b->target_f0};
    for (int k = 0; k < 6; k++) v.batch_targets[k] = tgt[k];
    const BatchCameras cams = batch_cameras_of(b);
    launch_begin(c, v, true, live_fresh, &cams, s);
    for (uint32_t f0 = 0; f0 < V && v.num_tasks; f0 += B) {
        v.batch_frame0 = f0, v.batch_frames = std::min(B, V - f0);
        hipLaunchKernelGGL(k_batch_chunk_begin, dim3(1), dim3(64), 0, s, v);
        launch_forward_chain(c, v, v.num_tasks * v.batch_frames, ForwardKernel::batch_grads, s);
        launch_backward_chain(c, v, v.num_tasks * v.batch_frames, true, s);
    }
    launch_grad_gather(c, v, import_into, s);
    hipLaunchKernelGGL(k_batch_epilogue, dim3(1), dim3(64), 0, s, v, V);
}

// egr_object_masks: the batch path's machinery for ONE view and ONE frame - camera table, control words, queues, live records - around k_forward_objects.
// No ray state (the variant keeps none), no k_finish*, no statistics reset, and the epilogue counts zero frames: total_num_calls, the framebuffer, both
// statistics, random_seeds and grads_enabled stay as they were. The frame draws its seeds from total_num_calls + 1, as the next launch would.
void egr_object_masks_launch(egr_context *c, const egr_object_mask_query *q, bool live_fresh, hipStream_t s) {
    egr_batch_reserve(c, 0u, 1u);
    if (c->object_bits_cap < c->g.count) { // the membership words in record order: grows with the cloud, freed by egr_destroy
        EGR_HIP(hipDeviceSynchronize());
        egr_dev_free(c, c->object_bits);
        c->object_bits_cap = 0;
        egr_dev_alloc(c, c->object_bits, (size_t)c->g.count);
        c->object_bits_cap = c->g.count;
    }
    DeviceView v = batch_view(c, 1u, 1u);
    v.team_help = 0; // single-wave workgroups always: nothing of the result may depend on timing
    v.batch_frame0 = 0u, v.batch_frames = 1u;
    ObjectBitList bits{};
    for (uint32_t j = 0; j < q->num_bits; j++) bits.bit[j] = q->bits[j];
    const ObjectQuery oq{c->object_bits, q->num_bits, q->masks, q->hit, q->top};
    egr_stamp_begin(c, "prologue+live", s);
    hipLaunchKernelGGL(k_batch_cameras, dim3(1), dim3(64), 0, s, q->rotation_c2w_dataset, q->camera_center, q->vertical_fov_radians, 1u, q->znear, q->zfar, c->batch_cams);
    hipLaunchKernelGGL(k_objects_prologue, dim3(1), dim3(64), 0, s, v);
    if (v.n && !live_fresh) hipLaunchKernelGGL(k_live, dim3((v.n + 255) / 256), dim3(256), 0, s, v, 0);
    if (v.n) hipLaunchKernelGGL(k_object_bits, dim3((v.n + 255u) / 256u), dim3(256), 0, s, v, q->row_bits, bits, q->num_bits, c->object_bits);
    egr_stamp_end(c, s);
    if (v.num_tasks) {
        egr_stamp_begin(c, "forward_objects", s);
        hipLaunchKernelGGL(k_forward_objects, dim3(chain_slots(c, v.num_tasks)), dim3(EGR_WAVE), (size_t)std::max<uint32_t>(q->num_bits, EGR_OBJ_MIN_SUMS) * EGR_WAVE * sizeof(float), s, v, oq);
        egr_stamp_end(c, s);
    }
    hipLaunchKernelGGL(k_batch_epilogue, dim3(1), dim3(64), 0, s, v, 0u);
}

void egr_export_step_hits(egr_context *c, int32_t *host_out, hipStream_t s) { export_per_step<int32_t, k_export_step_hits>(c, host_out, s); }
void egr_export_hit_hash(egr_context *c, uint64_t *host_out, hipStream_t s) { export_per_step<unsigned long long, k_export_hit_hash>(c, host_out, s); }

void egr_set_camera_launch(egr_context *c, const float *R, const float *centre, float fov, float znear, float zfar, hipStream_t s) {
    hipLaunchKernelGGL(k_set_camera, dim3(1), dim3(64), 0, s, c->cam, R, centre, fov, znear, zfar);
}
// R / centre in host memory (R_on_host / centre_on_host): read HERE, before the launch call returns, and handed over by value
void egr_set_camera_values_launch(egr_context *c, const float *R, bool R_on_host, const float *centre, bool centre_on_host, float fov, float znear, float zfar, hipStream_t s) {
    CameraPoseValues host{};
    if (R_on_host)
        for (int i = 0; i < 9; i++) host.R[i] = R[i];
    if (centre_on_host)
        for (int i = 0; i < 3; i++) host.centre[i] = centre[i];
    hipLaunchKernelGGL(k_set_camera_values, dim3(1), dim3(64), 0, s, c->cam, host, R_on_host ? nullptr : R, centre_on_host ? nullptr : centre, fov, znear, zfar);
}

void egr_upload_targets(egr_context *c, const float *const chw[6], hipStream_t s) {
    DeviceView v = egr_make_view(c);
    v.pixel_mask = nullptr; // (targets of every pixel of the rank's tiles, whatever a debug mask says)
    TargetImages t;
    for (int b = 0; b < 6; b++) t.chw[b] = chw[b];
    bool flat = c->world == 1 && v.num_pixels % 4 == 0 && v.num_pixels != 0;
    const float *const fbt[6] = {v.fb.target_diffuse, v.fb.target_specular, v.fb.target_depth, v.fb.target_normal, v.fb.target_roughness, v.fb.target_f0};
    for (int b = 0; b < 6; b++) flat = flat && ((reinterpret_cast<uintptr_t>(chw[b]) | reinterpret_cast<uintptr_t>(fbt[b])) & 15u) == 0;
    if (flat)
        hipLaunchKernelGGL(k_upload_targets_flat, dim3((unsigned)std::min<size_t>((v.num_pixels / 4 + 255) / 256, 4096)), dim3(256), 0, s, v, t);
    else if (v.num_tasks)
        hipLaunchKernelGGL(k_upload_targets, dim3(std::min(v.num_tasks, 65535u)), dim3(EGR_WAVE), 0, s, v, t);
}

void egr_copy_final_to_denoised(egr_context *c, hipStream_t s) {
    size_t n = (size_t)c->width * c->height * 3;
    hipLaunchKernelGGL(k_copy3, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, c->fb.output_final, c->fb.output_denoised, n);
}
