// k_forward_chain: scratch pointers, LDS and launch constants of a forward wave (included into the kernel body).
    const int lane = threadIdx.x & (EGR_WAVE - 1);
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); // this wave's place in its team (trace.hip: teams)
    const uint32_t slot = blockIdx.x * (uint32_t)TEAM + (uint32_t)wv;      // resident-wave slot: which candidate scratch / spill column is this wave's
    // candidate scratch of this resident wave: cand_cap entries per lane. Rounds 1-4 gave every lane a CONTIGUOUS run ([lane][k]: lanes append at their
    // own pace, a plain [k][lane] interleave dirtied a line per 4-B store - 4.4 KB written per ray - while a run lets the L2 merge 16 appends into one
    // line). What that cost was found at the end of round 5: every load of a selection scan touched 64 lines, 64 cycles of the CU's one address pipeline.
    // (keys: groups of four per lane, the lanes' groups interleaved - key k of lane l at ((k / 4) * 64 + l) * 4 + k % 4 of the wave's region - so the
    // 16-B load of a selection scan covers 1 KB of consecutive memory for the wave instead of 64 lines of 64 runs; EGR_KEY_AT)
    float *__restrict__ keys = v.cand_keys + (size_t)slot * EGR_WAVE * v.cand_cap;
#define EGR_KEY_AT(l, k) ((((size_t)((k) >> 2) * EGR_WAVE + (size_t)(l)) << 2) + ((k) & 3u))
#define EGR_KEY_Q(l, k) (reinterpret_cast<const float4 *>(keys)[(size_t)((k) >> 2) * EGR_WAVE + (size_t)(l)])
    // ((alpha, record) pairs likewise, in groups of two - entry k of lane l at ((k / 2) * 64 + l) * 2 + k % 2 - but only where the lanes append in step:
    // the lists of a PACKET step (primary tiles; `vals_il`, forward_task.inc). A pair walk appends to a ray's list over the whole walk, one entry here,
    // one there: in a contiguous run sixteen of them merge into one line in the L2, interleaved they dirty lines shared with seven other rays that are
    // written back half empty - trained-like forward chain 7.8-8.0 against 7.5 ms with the interleave everywhere.)
    float2 *__restrict__ vals = v.cand_vals + (size_t)slot * EGR_WAVE * v.cand_cap;
#define EGR_VAL_AT(l, k) (vals_il ? ((((size_t)((k) >> 1) * EGR_WAVE + (size_t)(l)) << 1) + ((k) & 1u)) : ((size_t)(l) * v.cand_cap + (k)))
#define EGR_VAL_Q(l, k) (reinterpret_cast<const float4 *>(vals + EGR_VAL_AT(l, k))[0]) // k even
    const uint4 *__restrict__ wnodes = v.wnodes;
    // pair walk (bounce steps): ONE wave-wide stack of (ray, node) pairs and ONE buffer of (ray, leaf) pairs per wave - no per-ray stacks,
    // queues or hand-out lists (every leaf a segment overlaps must be visited anyway, shaders.cu:69-71, so the order is free)
    __shared__ WalkShared wsh_all[TEAM];
    __shared__ TeamShared<TEAM> team;
    WalkShared &wsh = wsh_all[wv];
    uint32_t *const pstk = wsh.pstk, *const lbuf = wsh.lbuf, *const gcnt = wsh.gcnt, *const gtrav = wsh.gtrav, *const gext = wsh.gext, *const wc = wsh.wc;
    float4 (*const rayp)[3] = wsh.rayp;
    const float4 *__restrict__ app = v.app;

    const bool sentinels = __builtin_amdgcn_readfirstlane((int)*v.out_of_frame) != 0;
    const float exp_power = *v.cfg.exp_power;
    const float transmittance_threshold = *v.cfg.transmittance_threshold;
    const float backfacing_max_dist = *v.cfg.backfacing_max_dist;
    const float backfacing_thr = *v.cfg.backfacing_invalid_normal_threshold;
    const int num_bounces = OBJ ? 0 : min(*v.cfg.num_bounces, EGR_MAX_BOUNCES); // (k_forward_objects: the primary step only, whatever the config says)
    const float far_plane = *v.cam.zfar;
    const FwdConst fc{exp_power, transmittance_threshold, backfacing_max_dist, backfacing_thr, far_plane, num_bounces, sentinels, app, wnodes};
