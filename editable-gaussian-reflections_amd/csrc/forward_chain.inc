// k_forward_chain / k_forward_batch / k_forward_batch_grads / k_forward_objects: the kernel body (included into all four; expects GRADS, CUBE, TEAM, BATCH and
// OBJ - with OBJ the query `oq` and the wave's coverage sums `oacc`: the primary step only, no step epilogue). A wave takes
// tiles from the XCD queues and runs each through all its bounce steps. BATCH (the frames of egr_render_views, or with GRADS the views of egr_train_views,
// which then record hits into the batch's own arena and per-task tables, sized for tasks x frames): task index tq =
// ((macro-tile group) * batch_frames + frame) << task_shift | sub-task - the frames of one macro tile are adjacent, so the samples of a
// tile run close in time on one XCD (the queue chunks are contiguous task ranges). The tile's pixels come from the base task `tb`, its ray
// state from the full index.
#include "forward_decl.inc"
    if (lane < 4 * EGR_NSTEPS) wc[lane] = 0u;
    if (threadIdx.x == 0) team.done = 0u, team.hungry = 0u;
    if (threadIdx.x < TEAM) team.box_count[threadIdx.x] = 0u, team.busy[threadIdx.x] = 0u;
    __syncthreads(); // the kernel's only workgroup barrier: from here on the waves of a team run independently
    uint32_t cur_q = blockIdx.x & 7u;
    uint32_t arena_next = 0u, arena_end = 0u; // this wave's run of hit-arena blocks (forward_task.inc)

    for (;;) {
        const uint32_t tq = slot < v.num_slots ? wave_next_task(v.queues, BATCH ? v.num_tasks * v.batch_frames : v.num_tasks, cur_q, lane) : 0xFFFFFFFFu;
        if (tq == 0xFFFFFFFFu) break;
        uint32_t tb = tq;             // base task: the tile's pixels
        uint32_t bframe = 0u;         // (BATCH) batch frame index of this task
        const float *bcam = nullptr;  // (BATCH) its view's camera record
        if constexpr (BATCH) {
            const uint32_t grp = tq >> v.task_shift;
            tb = ((grp / v.batch_frames) << v.task_shift) | (tq & ((1u << v.task_shift) - 1u));
            bframe = v.batch_frame0 + grp % v.batch_frames;
            bcam = v.batch_cams + (size_t)(bframe / v.batch_spv) * EGR_BATCH_CAM_FLOATS;
        }
        const bool last_frame = !BATCH || bframe == v.batch_last_frame; // (stats / random_seeds are "last launch wins" stores)
        EGR_TIMES(unsigned long long chain_t[EGR_NSTEPS + 1] = {}; uint32_t chain_leaves = 0u;) EGR_TIMES_IS(9, chain_t[0] = __builtin_amdgcn_s_memrealtime();) // stamps of the WHOLE chain of a task (start, end of every step) for its first pixels
        EGR_STATS(const unsigned long long tchain0 = __builtin_amdgcn_s_memtime(); unsigned long long tepi = 0ull;)
        uint32_t bwd_cost = 0u; // (grad launches) what this tile's backward will cost, roughly in microseconds: 8 per primary hit row, 8 per 64 bounce hits + 2 per bounce hit row
        for (int step = 0; step <= num_bounces; step++) {
            do { // (a `continue` in the step body ends the step)
                const float near_plane = step == 0 ? *v.cam.znear : 0.0f; // forward_pass.cu:8-11
#include "forward_task.inc"
                const uint32_t a = wave_sum_u32(active ? 1u : 0u), b = wave_sum_u32(active ? traversed : 0u), c2 = wave_sum_u32(active ? nhits : 0u);
                const uint32_t d2 = wave_sum_u32(active ? cnt : 0u);
                if (lane == 0) wc[4 * step] += a, wc[4 * step + 1] += b, wc[4 * step + 2] += c2, wc[4 * step + 3] += d2;
                if (GRADS) {
                    const uint32_t rows = wave_max_u32(active ? nhits : 0u);
                    bwd_cost += step == 0 ? 8u * rows : c2 / 8u + 2u * rows;
                }
            } while (false);
            // R4 / R5 of this step for the tile's rays
            const TaskGeom etg = task_geom(v, tb, lane);
            EGR_STATS(const unsigned long long tepi0 = __builtin_amdgcn_s_memtime();)
            if (!OBJ && etg.inside) step_epilogue_lane(v, step, GRADS, num_bounces, etg, state_of(v, tq, lane), last_frame);
            EGR_STATS(tepi += __builtin_amdgcn_s_memtime() - tepi0;)
            EGR_TIMES_IS(9, chain_t[step + 1] = __builtin_amdgcn_s_memrealtime();)
        }
        if (GRADS && lane == 0) v.task_cost[tq] = bwd_cost;
        EGR_STATS(if (lane == 0) atomicAdd(diag64(v.control, DG_EPILOGUE_CYC), tepi), atomicAdd(diag64(v.control, DG_CHAIN_CYC), __builtin_amdgcn_s_memtime() - tchain0);)
        EGR_TIMES_IS(9,
            const TaskGeom ctg = task_geom(v, tb, lane);
            if (lane <= EGR_NSTEPS && ctg.inside) v.stats.num_traversed_per_pixel[ctg.pixel_id] = EGR_STAMP31(chain_t[lane]);
            if (lane == 4 && ctg.inside) v.stats.num_traversed_per_pixel[ctg.pixel_id] = (int32_t)chain_leaves;)
    }
    wave_sync();
    if (lane < EGR_NSTEPS) {
        add64(v.control, CW_RAYS + 2 * lane, wc[4 * lane]), add64(v.control, CW_CAND + 2 * lane, wc[4 * lane + 1]), add64(v.control, CW_COMP + 2 * lane, wc[4 * lane + 2]);
        add64(v.control, CW_ACCEPTED + 2 * lane, wc[4 * lane + 3]);
    }
    if (TEAM > 1 && v.team_help) {
        // no tiles left for this wave: it helps its team mates with the walks of theirs until all of them are through
        if (lane == 0) atomicAdd(&team.done, 1u);
        bool h_over = false;
        team_help_while<CUBE, TEAM>(v, fc, wsh_all, team, wv, blockIdx.x * (uint32_t)TEAM, h_over, [&]() { return uniform_u32(lds_peek(&team.done)) < (uint32_t)TEAM; });
        if (h_over) atomicOr(v.control + CW_STATUS, EGR_STATUS_CANDIDATE_OVERFLOW);
    }
