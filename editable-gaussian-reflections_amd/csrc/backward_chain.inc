// k_backward_chain / k_backward_batch: the kernel body (included into both; expects TEAM and BATCH). A wave takes tiles from the XCD queues in the order
// k_order_backward wrote and runs each tile's backward through all its steps (backward_task.inc). BATCH (the views of egr_train_views): the task index
// carries the frame as in k_forward_batch (((macro-tile group) * batch_frames + frame) << task_shift | sub-task); a task reads its frame's ray state, camera
// record, seed base and targets.
    const int lane = threadIdx.x & (EGR_WAVE - 1);
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    __shared__ uint32_t gt_keys_all[TEAM][EGR_GT_SLOTS];
    __shared__ __attribute__((aligned(16))) float gt_vals_all[TEAM][EGR_GT_STRIDE * EGR_GT_SLOTS];
    __shared__ uint32_t gt_claim_all[TEAM][EGR_GT_SLOTS]; // which lane adds to a slot in this round (backward_task.inc)
    __shared__ float4 stage_all[TEAM][4 * EGR_WAVE];     // records on their way out (wide_add_wave)
    __shared__ BwdTeamShared<TEAM> bteam;
    uint32_t *const gt_keys = gt_keys_all[wv], *const gt_claim = gt_claim_all[wv];
    float *const gt_vals = gt_vals_all[wv];
    float4 *const stage = stage_all[wv];
    if (threadIdx.x == 0) bteam.done = 0u;
    if (threadIdx.x < TEAM) bteam.ticket[threadIdx.x] = 0u, bteam.nitems[threadIdx.x] = 0u, bteam.finished[threadIdx.x] = 0u;
    uint32_t bepoch = 0u;
    // the two queues of the bounce steps live in the table's memory: the table is empty (flushed, all zero) while a tile's bounce steps run -
    // they come before its primary step - and the words they dirtied are cleared again before that step (backward_task.inc).
#define EGR_BQ_FLOATS (25 * EGR_WAVE) // floats of the table's memory the bounce steps use
    static_assert(EGR_GT_STRIDE * EGR_GT_SLOTS >= EGR_BQ_FLOATS, "the bounce queues must fit into the table");
    uint4 *bitems = reinterpret_cast<uint4 *>(gt_vals);  // [4 x 64] bounce steps: (ray, dL/dalpha, record, weight) of the hits of a chunk of four rows
    float *bdl = gt_vals + 16 * EGR_WAVE;                // [3 x 64] bounce steps: the rays' radiance gradient
    float *bray = gt_vals + 19 * EGR_WAVE;               // [6 x 64] bounce steps: the rays (origin, direction)
    for (int s = lane; s < EGR_GT_SLOTS; s += EGR_WAVE) gt_keys[s] = EGR_GT_EMPTY;
    for (int s = lane; s < EGR_GT_STRIDE * EGR_GT_SLOTS; s += EGR_WAVE) gt_vals[s] = 0.0f;
    __syncthreads(); // the kernel's only workgroup barrier (a team's waves run independently from here on)
    const float exp_power = *v.cfg.exp_power;
    const int num_bounces = min(*v.cfg.num_bounces, EGR_MAX_BOUNCES);
    const float view_size = BATCH ? 0.0f : tanf(*v.cam.vertical_fov_radians / 2.0f); // (primary_direction; a batch reads its view's record)
    uint32_t cur_q = blockIdx.x & 7u;
    uint32_t records = 0u; // 64-B gradient records this wave sent: bounce hits, primary hits without a table slot (two each), flushed table slots (two each) (egr_counters::bucket_records)

    for (;;) {
        const uint32_t tq = wave_next_task(v.queues + 8 * EGR_QUEUE_STRIDE, BATCH ? v.num_tasks * v.batch_frames : v.num_tasks, cur_q, lane);
        if (tq == 0xFFFFFFFFu) break;
        EGR_TIMES(unsigned long long bw_t0 = 0ull, bw_t1 = 0ull; uint32_t bw_rows0 = 0u;) EGR_TIMES_IS(8, bw_t0 = __builtin_amdgcn_s_memrealtime();) // stamps of a task's BACKWARD chain for its first pixels (tools/bwd_times.py)
        // The steps of a tile are independent in the backward (each reads its own arena chain and the forward's state, all gradients are
        // atomic adds), so their order is free: the PRIMARY step goes first and the bounce steps last - the bounce steps' batches are what
        // team mates can take (backward_task.inc), and team mates only have time once their own tiles are through, i.e. late in a heavy tile.
        bool table_dirty = false; // (wave-uniform) a bounce step used the table's memory for its queues
        {
            constexpr bool PRIMARY = true;
            const int step = 0;
            do {
#include "backward_task.inc"
            } while (false);
        }
        EGR_TIMES_IS(8, bw_t1 = __builtin_amdgcn_s_memrealtime();)
        for (int step = num_bounces; step >= 1; step--) {
            constexpr bool PRIMARY = false;
            do {
#include "backward_task.inc"
            } while (false);
        }
        if (table_dirty) { // (the table's memory held the bounce steps' queues: empty again for the next tile's primary step)
            EGR_BWD_SYNC();
            for (int s = lane; s < EGR_BQ_FLOATS; s += EGR_WAVE) gt_vals[s] = 0.0f;
            EGR_BWD_SYNC();
        }
        EGR_TIMES_IS(8,
            const unsigned long long bw_t2 = __builtin_amdgcn_s_memrealtime();
            const uint32_t bt = v.bwd_order[tq];
            const TaskGeom btg = task_geom(v, BATCH ? batch_base_task(v, bt) : bt, lane);
            if (btg.inside) {
                if (lane == 0) v.stats.num_traversed_per_pixel[btg.pixel_id] = EGR_STAMP31(bw_t0), v.stats.num_accumulated_per_pixel[btg.pixel_id] = EGR_STAMP31(bw_t2);
                if (lane == 1) v.stats.num_traversed_per_pixel[btg.pixel_id] = EGR_STAMP31(bw_t1), v.stats.num_accumulated_per_pixel[btg.pixel_id] = (int32_t)bw_rows0;
            })
    }
    if constexpr (TEAM > 1) {
        // no tiles left: this wave takes batches of bounce hits its team mates have queued until all of them are through
        if (lane == 0) atomicAdd(&bteam.done, 1u);
        records += bwd_team_help<TEAM>(v, exp_power, bteam, gt_vals_all, stage, wv, lane);
    }
    if (lane == 0 && records) atomicAdd(v.control + CW_BUCKET_RECORDS, records);
