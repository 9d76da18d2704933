// The backward chain of k_backward_chain / k_backward_batch: a wave takes tiles from the XCD queues in the order k_order_backward wrote and runs each
// tile's backward through all its steps (backward_chain -> backward_step: B1 output gradients, B2 per-hit chain newest first, gradient table flush).
// BATCH (the views of egr_train_views): the task index carries the frame as in k_forward_batch (trace.hip: ChainTask); a task reads its frame's ray
// state, camera record, seed base and targets.
//
// Included by trace.hip once, inside its anonymous namespace. From the definitions above the include it uses: wave_next_task, wave_max_u32, uniform_u32,
// ChainTask / decode_task, primary_ray, wave_sync (EGR_BWD_SYNC), lds_peek, lds_poke, the table and record constants (EGR_GT_*, EGR_REC*, PC_*),
// wide_add_wave, grad_table_flush, primary_table_add, hit_geometry_fn, bounce_batch, BwdTeamShared and bwd_team_help; from
// egr_state.hpp task_geom and state_of; from egr_diag.hpp the EGR_STATS / EGR_TIMES statement macros.
#pragma once

// the two queues of the bounce steps live in the table's memory: the table is empty (flushed, all zero) while a tile's bounce steps run -
// they come before its primary step - and the words they dirtied are cleared again before that step (backward_chain).
constexpr int BOUNCE_QUEUE_FLOATS = 25 * EGR_WAVE; // floats of the table's memory the bounce steps use
static_assert(EGR_GT_STRIDE * EGR_GT_SLOTS >= BOUNCE_QUEUE_FLOATS, "the bounce queues must fit into the table");

// LDS and launch constants of a backward wave.
template <int TEAM> struct BwdWave {
    int lane, wv;
    uint32_t *gt_keys; // the primary step's table of this wave (trace.hip: primary_table_add)
    float *gt_vals;
    uint32_t *gt_claim; // per slot: the last lane of the current row that came to it (empty between rows)
    float4 *stage;      // records on their way out (wide_add_wave)
    BwdTeamShared<TEAM> &bteam;
    uint4 *bitems; // [4 x 64] bounce steps: (ray, dL/dalpha, record, weight) of the hits of a chunk of four rows
    float *bdl;    // [3 x 64] bounce steps: the rays' radiance gradient
    float *bray;   // [6 x 64] bounce steps: the rays (origin, direction)
    float exp_power;
    int num_bounces;
    float view_size;  // (primary_direction; a batch reads its view's record)
    uint32_t bepoch;  // epoch of this wave's ticket (bounce_hits)
    bool table_dirty; // (wave-uniform) a bounce step of the current tile used the table's memory for its queues
};

// What the EGR_TASK_TIMES = 8 build (egr_diag.hpp) carries along a task's backward chain: its stamps and the primary step's rows for the tile's first
// pixels (tools/bwd_times.py). Empty in the product build.
struct BwdDiag {
    EGR_TIMES(unsigned long long bw_t0 = 0ull, bw_t1 = 0ull; uint32_t bw_rows0 = 0u;)
};

struct RayGrads { // B1: what is constant along this lane's ray of a step
    f3 dL_rgb, dL_n, dL_f0;
    float dL_depth, dL_rough;
    f3 ro, rd;
    f3 rem_rgb, rem_n, rem_f0;
    float rem_depth, rem_rough, T_minus_Ttot;
};

// ---- B1: output gradients (backward_pass.cu:80-108); constant along the ray ----------------------
template <bool PRIMARY, bool BATCH, int TEAM>
EGR_DI RayGrads output_gradients(const DeviceView &v, const BwdWave<TEAM> &W, const ChainTask &task, const TaskGeom &tg, const StateRef &S, const int step,
                                 const uint32_t steps_done, const uint32_t nhits) {
    RayGrads g{mk3(0, 0, 0), mk3(0, 0, 0), mk3(0, 0, 0), 0.0f, 0.0f, mk3(0, 0, 0), mk3(0, 0, 1), mk3(0, 0, 0), mk3(0, 0, 0), mk3(0, 0, 0), 0.0f, 0.0f, 0.0f};
    if (nhits > 0) {
        const uint32_t pid = tg.pixel_id;
        const float third = 1.0f / 3.0f;
        if constexpr (PRIMARY) {
            f3 o_rgb = S.ld3(SF(0, S_RGB)), o_n = S.ld3(SF(0, S_NORMAL)), o_f0 = S.ld3(SF(0, S_F0));
            float o_depth = S.ld(SF(0, S_DEPTH)), o_rough = S.ld(SF(0, S_ROUGH));
            if constexpr (BATCH) {
                // the view's own targets (channel-major [V][C][H][W]; NULL: zeros) - the same operations as below on the same values
                const size_t P = v.num_pixels;
                const uint32_t bframe = task.bframe;
                auto tgt = [&](int b, uint32_t ch, uint32_t c) { const float *p = v.batch_targets[b]; return p ? p[((size_t)bframe * ch + c) * P + pid] : 0.0f; };
                g.dL_rgb = mk3(third * sign1(o_rgb.x - tgt(0, 3, 0)), third * sign1(o_rgb.y - tgt(0, 3, 1)), third * sign1(o_rgb.z - tgt(0, 3, 2))) * *v.cfg.loss_weight_diffuse;
                g.dL_depth = sign1(o_depth - tgt(2, 1, 0)) * *v.cfg.loss_weight_depth;
                g.dL_n = mk3(third * sign1(o_n.x - tgt(3, 3, 0)), third * sign1(o_n.y - tgt(3, 3, 1)), third * sign1(o_n.z - tgt(3, 3, 2))) * *v.cfg.loss_weight_normal;
                g.dL_f0 = mk3(third * sign1(o_f0.x - tgt(5, 3, 0)), third * sign1(o_f0.y - tgt(5, 3, 1)), third * sign1(o_f0.z - tgt(5, 3, 2))) * *v.cfg.loss_weight_f0;
                g.dL_rough = sign1(o_rough - tgt(4, 1, 0)) * *v.cfg.loss_weight_roughness;
            } else {
                // the framebuffer's pixel-major buffers, or the caller's channel-major images in place (NULL: zeros): one set of loads, two launch-uniform strides
                const bool planes = v.target_planes != 0u;
                const size_t cs = planes ? (size_t)v.num_pixels : (size_t)1;
                auto tgt = [&](int b, uint32_t ch, uint32_t c) { const float *p = v.batch_targets[b]; return p ? p[(size_t)pid * (planes ? 1u : ch) + c * cs] : 0.0f; };
                g.dL_rgb = mk3(third * sign1(o_rgb.x - tgt(0, 3, 0)), third * sign1(o_rgb.y - tgt(0, 3, 1)), third * sign1(o_rgb.z - tgt(0, 3, 2))) * *v.cfg.loss_weight_diffuse;
                g.dL_depth = sign1(o_depth - tgt(2, 1, 0)) * *v.cfg.loss_weight_depth;
                g.dL_n = mk3(third * sign1(o_n.x - tgt(3, 3, 0)), third * sign1(o_n.y - tgt(3, 3, 1)), third * sign1(o_n.z - tgt(3, 3, 2))) * *v.cfg.loss_weight_normal;
                g.dL_f0 = mk3(third * sign1(o_f0.x - tgt(5, 3, 0)), third * sign1(o_f0.y - tgt(5, 3, 1)), third * sign1(o_f0.z - tgt(5, 3, 2))) * *v.cfg.loss_weight_f0;
                g.dL_rough = sign1(o_rough - tgt(4, 1, 0)) * *v.cfg.loss_weight_roughness;
            }
            // the primary ray is regenerated from the seed instead of being stored (a batch: its view's camera record and the seed base of its frame)
            const PrimaryRay p = primary_ray<BATCH>(v, tg, task, W.view_size);
            g.ro = p.ro, g.rd = p.rd;
        } else {
            f3 spec = mk3(0, 0, 0);
            for (int j = 1; j < W.num_bounces + 1; j++)
                if ((uint32_t)j < steps_done) spec = spec + S.ld3(SF(j, S_RGB)); // unexecuted steps hold 0 upstream
            f3 t_spec;
            if constexpr (BATCH) {
                const float *p = v.batch_targets[1];
                const size_t P = v.num_pixels, q = (size_t)task.bframe * 3 * P + pid;
                t_spec = p ? mk3(p[q], p[q + P], p[q + 2 * P]) : mk3(0, 0, 0);
            } else {
                const float *p = v.batch_targets[1]; // (pixel-major or planes, as the primary step's)
                const size_t q = (size_t)pid * (v.target_planes ? 1u : 3u), cs = v.target_planes ? (size_t)v.num_pixels : (size_t)1;
                t_spec = p ? mk3(p[q], p[q + cs], p[q + 2 * cs]) : mk3(0, 0, 0);
            }
            float down = powf(1.0f - S.ld(SF(step - 1, S_ROUGH)), EGR_ROUGHNESS_DOWNWEIGHT_GRAD_POWER); // :11-13
            g.dL_rgb = (mk3(third * sign1(spec.x - t_spec.x), third * sign1(spec.y - t_spec.y), third * sign1(spec.z - t_spec.z)) *
                        *v.cfg.loss_weight_specular) * down;
            g.dL_rgb = g.dL_rgb * S.ld3(SF(step - 1, S_THR)); // :107, throughput of the previous step
            g.ro = S.ld3(SF(step - 1, S_NEXT_O));
            g.rd = S.ld3(SF(step - 1, S_NEXT_D));
        }
        g.rem_rgb = S.ld3(SF(step, S_REM_RGB)), g.rem_n = S.ld3(SF(step, S_REM_NORMAL)), g.rem_f0 = S.ld3(SF(step, S_REM_F0));
        g.rem_depth = S.ld(SF(step, S_REM_DEPTH)), g.rem_rough = S.ld(SF(step, S_REM_ROUGH));
        g.T_minus_Ttot = S.ld(SF(step, S_T)) - S.ld(SF(step, S_TTOT));
    }
    return g;
}

// ---- B2 of a BOUNCE step in two passes per chunk of four hit rows. A row of the arena holds the it-th hit of every ray, and rays
// end at different depths: with one lane per RAY a row costs the full per-hit arithmetic however few rays still have a hit (58 %
// of the lanes on the bounce steps of the trained-like cloud; half of that again with 8x4-pixel tasks). Only the suffix sums that
// give dL/dalpha run along the ray; the geometry gradient of a hit (nine tenths of the arithmetic) needs dL/dalpha and nothing
// else from its neighbours. Pass 1 (lane = ray) walks the chunk's rows newest first and queues (ray, row, dL/dalpha) per hit in
// LDS; pass 2 (lane = HIT, 64 at a time whatever ray they belong to) does the geometry and sends the 14 components as one wide add.
// `blk`: the newest block of the tile's arena chain of this step. Returns the records sent.
template <int TEAM> EGR_DI uint32_t bounce_hits(const DeviceView &v, BwdWave<TEAM> &W, const RayGrads &g, uint32_t blk, const uint32_t nhits, const uint32_t max_hits) {
    const int lane = W.lane, wv = W.wv;
    const float exp_power = W.exp_power;
    BwdTeamShared<TEAM> &bteam = W.bteam;
    uint4 *const bitems = W.bitems;
    float *const bdl = W.bdl, *const bray = W.bray;
    float4 *const stage = W.stage;
    const f3 dL_rgb = g.dL_rgb, ro = g.ro, rd = g.rd, rem_rgb = g.rem_rgb;
    const float T_minus_Ttot = g.T_minus_Ttot;
    uint32_t records = 0u;
    W.table_dirty = true;
    bdl[lane] = dL_rgb.x, bdl[EGR_WAVE + lane] = dL_rgb.y, bdl[2 * EGR_WAVE + lane] = dL_rgb.z;
    bray[lane] = ro.x, bray[EGR_WAVE + lane] = ro.y, bray[2 * EGR_WAVE + lane] = ro.z, bray[3 * EGR_WAVE + lane] = rd.x, bray[4 * EGR_WAVE + lane] = rd.y, bray[5 * EGR_WAVE + lane] = rd.z;
    f3 prev_rgb = mk3(0, 0, 0), w_rgb = mk3(0, 0, 0);
    const uint32_t nblocks = (max_hits + EGR_HIT_BLOCK_ROWS - 1) / EGR_HIT_BLOCK_ROWS;
    EGR_BWD_SYNC();
    for (uint32_t b = nblocks; b-- > 0;) {
        const float4 *rows = v.hit_arena + (size_t)blk * (EGR_HIT_BLOCK_ROWS + 1) * EGR_WAVE;
        for (int chunk = EGR_HIT_BLOCK_ROWS / 4 - 1; chunk >= 0; chunk--) {
            uint32_t nitems = 0u; // wave-uniform
            // the chunk's fetches first - four arena records, then the four appearance quarters they name: two round trips per chunk instead
            // of eight (rows past a ray's last hit are read and ignored: the block's rows all exist)
            float4 rec4[4], a04[4];
#pragma unroll
            for (int r4 = 0; r4 < 4; r4++) rec4[r4] = rows[(size_t)(1 + 4 * chunk + r4) * EGR_WAVE + lane];
#pragma unroll
            for (int r4 = 0; r4 < 4; r4++) a04[r4] = v.app[2 * ((b * EGR_HIT_BLOCK_ROWS + (uint32_t)(4 * chunk + r4)) < nhits ? f2u(rec4[r4].x) : 0u)];
#pragma unroll
            for (int r4 = 3; r4 >= 0; r4--) {
                const int row = 4 * chunk + r4;
                const uint32_t it = b * EGR_HIT_BLOCK_ROWS + (uint32_t)row;
                const bool act = it < nhits;
                float dL_dalpha = 0.0f, weight = 0.0f;
                uint32_t pos = 0u;
                if (act) {
                    const float4 rec = rec4[r4];
                    pos = f2u(rec.x);
                    const float alpha = rec.z, transmittance = rec.w;
                    weight = (float)((double)transmittance / (1.0 - (double)alpha) * (double)alpha); // :111
                    const float4 a0 = a04[r4];
                    const f3 g_rgb = mk3(a0.x, a0.y, a0.z);
                    w_rgb = w_rgb + (g_rgb - prev_rgb) * transmittance; // :118-132 (a bounce step only carries the radiance)
                    prev_rgb = g_rgb;
                    const float one_m_alpha = 1.0f - alpha, r1ma = egr_rcp_refined(one_m_alpha); // (both quotients below from one refined reciprocal)
                    const float tmp1 = egr_div_rn(1.0f, one_m_alpha, r1ma); // :134-148
                    dL_dalpha += dot(w_rgb * tmp1, dL_rgb);
                    const float tmp2 = -egr_div_rn(T_minus_Ttot, one_m_alpha, r1ma);
                    dL_dalpha += tmp2 * dot(rem_rgb, dL_rgb);
                }
                const unsigned long long am = __ballot(act);
                if (act) bitems[nitems + __builtin_amdgcn_mbcnt_hi((uint32_t)(am >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)am, 0u))] = make_uint4((uint32_t)lane, f2u(dL_dalpha), pos, f2u(weight));
                nitems += (uint32_t)__popcll(am);
            }
            if (nitems == 0u) continue;
            EGR_BWD_SYNC();
            const uint32_t nbatch = (nitems + (uint32_t)EGR_WAVE - 1u) / (uint32_t)EGR_WAVE;
            if constexpr (TEAM > 1) {
                // the chunk's batches of 64 hits are taken one by one from a ticket in LDS - by this wave and by every team mate that has
                // no tile left (bwd_team_help): a hit needs nothing but its queue item, the rays and radiance gradients in this wave's LDS
                // and its gaussian's records; the gradients are atomic adds whoever sends them
                if (lane == 0) {
                    lds_poke(&bteam.finished[wv], 0u);
                    lds_poke(&bteam.nitems[wv], nitems);
                    W.bepoch = (W.bepoch + 1u) & 0xFFFu;
                    lds_poke(&bteam.ticket[wv], (W.bepoch << 20) | (nbatch << 10)); // (after the queue, the counters: LDS keeps a wave's order)
                }
                for (;;) {
                    uint32_t tk = 0u;
                    if (lane == 0) tk = atomicAdd(&bteam.ticket[wv], 1u);
                    tk = uniform_u32(tk);
                    const uint32_t bi = tk & 0x3FFu;
                    if (bi >= nbatch) break;
                    records += bounce_batch(v, exp_power, bitems, bdl, bray, bi * (uint32_t)EGR_WAVE, nitems, stage, lane);
                    if (lane == 0) atomicAdd(&bteam.finished[wv], 1u);
                }
                while (uniform_u32(lds_peek(&bteam.finished[wv])) < nbatch) __builtin_amdgcn_s_sleep(1); // batches team mates still work on
            } else {
                for (uint32_t bi = 0; bi < nbatch; bi++) records += bounce_batch(v, exp_power, bitems, bdl, bray, bi * (uint32_t)EGR_WAVE, nitems, stage, lane);
            }
            EGR_BWD_SYNC(); // the queue is reused by the next chunk
        }
        blk = f2u(rows[0].x); // header: previous (older) block of this chain
    }
    return records;
}

// ---- B2 of the PRIMARY step: the per-hit chain, newest hit first, through the wave's LDS table, and the table's flush (one per tile). The geometry
// half of a hit (trace.hip: hit_geometry_fn) - opacity, mean and the six components of Q from the record position, the ray, the live (.., opacity,
// sigma) quarter and dL/dalpha - is independent of the other hits of the ray; the sequential half (suffix sums -> dL/dalpha) runs here.
// `blk`: the newest block of the tile's arena chain of this step. Returns the records sent.
template <int TEAM> EGR_DI uint32_t primary_hits(const DeviceView &v, BwdWave<TEAM> &W, const RayGrads &g, uint32_t blk, const uint32_t nhits, const uint32_t max_hits) {
    const int lane = W.lane;
    uint32_t *const gt_keys = W.gt_keys, *const gt_claim = W.gt_claim;
    float *const gt_vals = W.gt_vals;
    float4 *const stage = W.stage;
    const f3 dL_rgb = g.dL_rgb, dL_n = g.dL_n, dL_f0 = g.dL_f0, ro = g.ro, rd = g.rd, rem_rgb = g.rem_rgb, rem_n = g.rem_n, rem_f0 = g.rem_f0;
    const float dL_depth = g.dL_depth, dL_rough = g.dL_rough, rem_depth = g.rem_depth, rem_rough = g.rem_rough, T_minus_Ttot = g.T_minus_Ttot;
    uint32_t records = 0u;
    f3 prev_rgb = mk3(0, 0, 0), w_rgb = mk3(0, 0, 0), prev_n = mk3(0, 0, 0), w_n = mk3(0, 0, 0), prev_f0 = mk3(0, 0, 0), w_f0 = mk3(0, 0, 0);
    float prev_rough = 0, w_rough = 0, prev_depth = 0, w_depth = 0;
    const uint32_t nblocks = (max_hits + EGR_HIT_BLOCK_ROWS - 1) / EGR_HIT_BLOCK_ROWS;
    EGR_STATS(unsigned long long bt_math = 0ull, bt_table = 0ull, bt_wide = 0ull, bt_rows = 0ull;) // s_memtime per phase of a hit row: [math, neighbour combine + LDS table, wide adds] + the tile's table flush
    EGR_STATS(unsigned long long bt_lanes = 0ull, bt_steps = 0ull, bt_leaders = 0ull;) // of the rows' groups (trace.hip: primary_table_add): lanes with a hit, pointer-jumping steps, leaders
    for (uint32_t b = nblocks; b-- > 0;) {
        const float4 *rows = v.hit_arena + (size_t)blk * (EGR_HIT_BLOCK_ROWS + 1) * EGR_WAVE;
        int pf_row = -1; // the row of this block whose arena entry `rec_pf` holds (requested while the row before it was worked off)
        float4 rec_pf = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int row = EGR_HIT_BLOCK_ROWS - 1; row >= 0; row--) {
            const uint32_t it = b * EGR_HIT_BLOCK_ROWS + (uint32_t)row;
            if (it >= max_hits) continue;
            // a hit without a table slot leaves the divergent block with its gradients in `gx`: the wide add that follows is a wave-level operation
            bool direct = false, want = false; // want: this lane holds a hit of this row
            uint32_t dpos = 0;
            float gx[EGR_GT_COMPS]; // this hit's gradient components, PC_* order (what leaves the lane when `direct`: a primary hit without a table slot)
            EGR_STATS(const unsigned long long bt0 = __builtin_amdgcn_s_memtime(); unsigned long long bt1 = bt0; bt_rows++;)
            // a row costs two dependent round trips - its arena entry, then the records the entry names: the NEXT row's entry is requested now
            // (the request comes first and the rare direct load - the first row of a block - completes inside its own branch: with the two the other
            // way round the compiler cannot tell how many loads are in flight where the entry is first used and waits for all of them)
            float4 rec_cur = rec_pf;
            const bool have_pf = pf_row == row; // wave-uniform
            if (row > 0) {
                if (it <= nhits) rec_pf = rows[(size_t)row * EGR_WAVE + lane]; // (row - 1 holds hit it - 1 < nhits)
                pf_row = row - 1;
            }
            if (!have_pf) {
                if (it < nhits) rec_cur = rows[(size_t)(1 + row) * EGR_WAVE + lane];
#if defined(__HIP_DEVICE_COMPILE__)
                asm volatile("" ::"v"(rec_cur.x), "v"(rec_cur.y), "v"(rec_cur.z), "v"(rec_cur.w));
#endif
            }
            if (it < nhits) {
                const float4 rec = rec_cur;
                const uint32_t pos = f2u(rec.x);          // record index (sorted position)
                const float distance = rec.y, alpha = rec.z, transmittance = rec.w;
                const float4 a0 = v.app[2 * pos], a1 = v.app[2 * pos + 1], a2 = v.inst_w[4 * pos + 3];
                const f3 g_rgb = mk3(a0.x, a0.y, a0.z);
                const float weight = (float)((double)transmittance / (1.0 - (double)alpha) * (double)alpha); // :111
                // activation backward is evaluated on the ACTIVATED value (activations.cu:29,41-43) -> pass-through
                f3 d_rgb = (dL_rgb * weight);
                f3 d_n = dL_n * weight, d_f0 = dL_f0 * weight;
                float d_rough = dL_rough * weight;

                w_rgb = w_rgb + (g_rgb - prev_rgb) * transmittance; // :118-132
                prev_rgb = g_rgb;
                {
                    f3 g_n = mk3(a0.w, a1.x, a1.y), g_f0 = mk3(a1.z, a1.w, a2.x);
                    w_n = w_n + (g_n - prev_n) * transmittance;
                    prev_n = g_n;
                    w_f0 = w_f0 + (g_f0 - prev_f0) * transmittance;
                    prev_f0 = g_f0;
                    w_rough += (a2.y - prev_rough) * transmittance;
                    prev_rough = a2.y;
                    w_depth += (distance - prev_depth) * transmittance;
                    prev_depth = distance;
                }
                float dL_dalpha = 0.0f; // :134-148
                const float one_m_alpha = 1.0f - alpha, r1ma = egr_rcp_refined(one_m_alpha); // (both quotients below from one refined reciprocal)
                const float tmp1 = egr_div_rn(1.0f, one_m_alpha, r1ma);
                dL_dalpha += dot(w_rgb * tmp1, dL_rgb);
                dL_dalpha += dot(w_n * tmp1, dL_n);
                dL_dalpha += dot(w_f0 * tmp1, dL_f0);
                dL_dalpha += (w_rough * tmp1) * dL_rough;
                dL_dalpha += (w_depth * tmp1) * dL_depth;
                const float tmp2 = -egr_div_rn(T_minus_Ttot, one_m_alpha, r1ma);
                dL_dalpha += tmp2 * dot(rem_rgb, dL_rgb);
                dL_dalpha += tmp2 * dot(rem_n, dL_n);
                dL_dalpha += tmp2 * dot(rem_f0, dL_f0);
                dL_dalpha += tmp2 * (rem_rough * dL_rough);
                dL_dalpha += tmp2 * (rem_depth * dL_depth);

                hit_geometry_fn(v, W.exp_power, pos, a2, ro, rd, dL_dalpha, gx); // opacity, mean, Q
                gx[PC_RGB] = d_rgb.x, gx[PC_RGB + 1] = d_rgb.y, gx[PC_RGB + 2] = d_rgb.z, gx[PC_WEIGHT] = weight;
                gx[PC_NORMAL] = d_n.x, gx[PC_NORMAL + 1] = d_n.y, gx[PC_NORMAL + 2] = d_n.z;
                gx[PC_F0] = d_f0.x, gx[PC_F0 + 1] = d_f0.y, gx[PC_F0 + 2] = d_f0.z, gx[PC_ROUGH] = d_rough;
                EGR_STATS(bt1 = __builtin_amdgcn_s_memtime();)
                // primary hits go through the wave's LDS table (trace.hip: primary_table_add below, outside this divergent block: the row's sums pull
                // across the wave, and a full table is emptied by the whole wave). (Bounce tiles are incoherent - an LDS table removed only 25 % of the
                // contributions at 15 ds_add_f32 per hit: bounce_batch sends a hit's 14 components straight to the gradient row as one record.)
                dpos = pos;
                want = true;
            }
            uint32_t jump_steps, row_leaders;
            direct = primary_table_add(v, want, dpos, gx, gt_keys, gt_vals, gt_claim, stage, lane, records, jump_steps, row_leaders);
            EGR_STATS(bt_lanes += (unsigned long long)__popcll(__ballot(want)); bt_steps += jump_steps; bt_leaders += row_leaders;)
            EGR_STATS(const unsigned long long bt2 = __builtin_amdgcn_s_memtime(); bt_math += bt1 - bt0; bt_table += bt2 - bt1;)
            if (__ballot(direct) != 0ull) {
                float lo[EGR_REC0_COMPS], hi[EGR_REC1_COMPS]; // one record per segment of the row, like a flushed slot
#pragma unroll
                for (int c = 0; c < EGR_REC0_COMPS; c++) lo[c] = gx[c];
#pragma unroll
                for (int c = 0; c < EGR_REC1_COMPS; c++) hi[c] = gx[EGR_REC0_COMPS + c];
                wide_add_wave<EGR_REC0_CELL>(v, direct, dpos, lo, stage);
                wide_add_wave<EGR_REC1_CELL>(v, direct, dpos, hi, stage);
                records += 2u * (uint32_t)__popcll(__ballot(direct));
            }
            EGR_STATS(bt_wide += __builtin_amdgcn_s_memtime() - bt2;)
        }
        blk = f2u(rows[0].x); // header: previous (older) block of this chain
    }
    EGR_STATS(const unsigned long long bt3 = __builtin_amdgcn_s_memtime();)
    records += grad_table_flush(v, gt_keys, gt_vals, stage, lane); // one flush per tile
    EGR_STATS(if (lane == 0) {
        unsigned long long *d = diag64(v.control, DG_BWD_MATH_CYC);
        atomicAdd(d, bt_math), atomicAdd(d + 1, bt_table), atomicAdd(d + 2, bt_wide), atomicAdd(d + 3, __builtin_amdgcn_s_memtime() - bt3), atomicAdd(d + 4, bt_rows);
        unsigned long long *r = diag64(v.control, DG_BWD_ROW_GROUPS);
        atomicAdd(r, bt_lanes), atomicAdd(r + 1, bt_steps), atomicAdd(r + 2, bt_leaders);
    })
    return records;
}

// The backward of ONE step of ONE tile; `tq`: the tile's place in the backward order. Returns the 64-B gradient records sent.
template <bool PRIMARY, int TEAM, bool BATCH> EGR_DI uint32_t backward_step(const DeviceView &v, BwdWave<TEAM> &W, const uint32_t tq, const int step, BwdDiag &D) {
    const int lane = W.lane;
    const uint32_t tqo = v.bwd_order[tq]; // (costliest tasks of the queue's chunk first: k_order_backward)
    const uint32_t blk = v.task_last_block[(size_t)step * (BATCH ? v.num_tasks * v.batch_frames : v.num_tasks) + tqo]; // the tile's arena chain of this step (wave-uniform)
    if (blk == 0xFFFFFFFFu) return 0u;
    const ChainTask task = decode_task<BATCH>(v, tqo); // (BATCH) the tile's pixels; the task's batch frame = its view (egr_train_views: one sample per view)
    const TaskGeom tg = task_geom(v, task.tb, lane);
    const StateRef S = state_of(v, task.tq, lane);
    const uint32_t steps_done = tg.inside ? f2u(S.ld(F_STEPS)) : 0u;
    const uint32_t nhits = (tg.inside && (uint32_t)step < steps_done && blk != 0xFFFFFFFFu) ? f2u(S.ld(SF(step, S_NHITS))) : 0u; // shaders.cu:157-158
    const uint32_t max_hits = wave_max_u32(nhits);
    if (max_hits == 0) return 0u;
    EGR_TIMES_IS(8, if (PRIMARY) D.bw_rows0 = max_hits;)
    const RayGrads g = output_gradients<PRIMARY, BATCH>(v, W, task, tg, S, step, steps_done, nhits);
    if constexpr (PRIMARY) return primary_hits(v, W, g, blk, nhits, max_hits);
    else return bounce_hits(v, W, g, blk, nhits, max_hits);
}

// The kernel body of the two backward chain kernels.
template <int TEAM, bool BATCH> EGR_DI void backward_chain(const DeviceView v) {
    const int lane = threadIdx.x & (EGR_WAVE - 1);
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    __shared__ uint32_t gt_keys_all[TEAM][EGR_GT_SLOTS];
    __shared__ __attribute__((aligned(16))) float gt_vals_all[TEAM][EGR_GT_STRIDE * EGR_GT_SLOTS];
    __shared__ uint32_t gt_claim_all[TEAM][EGR_GT_SLOTS];
    __shared__ float4 stage_all[TEAM][4 * EGR_WAVE];
    __shared__ BwdTeamShared<TEAM> bteam;
    if (threadIdx.x == 0) bteam.done = 0u;
    if (threadIdx.x < TEAM) bteam.ticket[threadIdx.x] = 0u, bteam.nitems[threadIdx.x] = 0u, bteam.finished[threadIdx.x] = 0u;
    uint32_t *const gt_keys = gt_keys_all[wv];
    float *const gt_vals = gt_vals_all[wv];
    for (int s = lane; s < EGR_GT_SLOTS; s += EGR_WAVE) gt_keys[s] = EGR_GT_EMPTY, gt_claim_all[wv][s] = EGR_GT_EMPTY;
    for (int s = lane; s < EGR_GT_STRIDE * EGR_GT_SLOTS; s += EGR_WAVE) gt_vals[s] = 0.0f;
    __syncthreads(); // the kernel's only workgroup barrier (a team's waves run independently from here on)
    const float exp_power = *v.cfg.exp_power;
    const int num_bounces = min(*v.cfg.num_bounces, EGR_MAX_BOUNCES);
    const float view_size = BATCH ? 0.0f : tanf(*v.cam.vertical_fov_radians / 2.0f);
    BwdWave<TEAM> W{lane, wv, gt_keys, gt_vals, gt_claim_all[wv], stage_all[wv], bteam, reinterpret_cast<uint4 *>(gt_vals), gt_vals + 16 * EGR_WAVE, gt_vals + 19 * EGR_WAVE,
                    exp_power, num_bounces, view_size, 0u, false};
    uint32_t cur_q = blockIdx.x & 7u;
    uint32_t records = 0u; // 64-B gradient records this wave sent: bounce hits, primary hits without a table slot (two each), flushed table slots (two each) (egr_counters::bucket_records)

    for (;;) {
        const uint32_t tq = wave_next_task(v.queues + 8 * EGR_QUEUE_STRIDE, BATCH ? v.num_tasks * v.batch_frames : v.num_tasks, cur_q, lane);
        if (tq == 0xFFFFFFFFu) break;
        BwdDiag D;
        EGR_TIMES_IS(8, D.bw_t0 = __builtin_amdgcn_s_memrealtime();)
        // The steps of a tile are independent in the backward (each reads its own arena chain and the forward's state, all gradients are
        // atomic adds), so their order is free: the PRIMARY step goes first and the bounce steps last - the bounce steps' batches are what
        // team mates can take (bounce_hits), and team mates only have time once their own tiles are through, i.e. late in a heavy tile.
        W.table_dirty = false;
        records += backward_step<true, TEAM, BATCH>(v, W, tq, 0, D);
        EGR_TIMES_IS(8, D.bw_t1 = __builtin_amdgcn_s_memrealtime();)
        for (int step = num_bounces; step >= 1; step--) records += backward_step<false, TEAM, BATCH>(v, W, tq, step, D);
        if (W.table_dirty) { // (the table's memory held the bounce steps' queues: empty again for the next tile's primary step)
            EGR_BWD_SYNC();
            for (int s = lane; s < BOUNCE_QUEUE_FLOATS; s += EGR_WAVE) gt_vals[s] = 0.0f;
            EGR_BWD_SYNC();
        }
        EGR_TIMES_IS(8,
            const unsigned long long bw_t2 = __builtin_amdgcn_s_memrealtime();
            const TaskGeom btg = task_geom(v, decode_task<BATCH>(v, v.bwd_order[tq]).tb, lane);
            if (btg.inside) {
                if (lane == 0) v.stats.num_traversed_per_pixel[btg.pixel_id] = EGR_STAMP31(D.bw_t0), v.stats.num_accumulated_per_pixel[btg.pixel_id] = EGR_STAMP31(bw_t2);
                if (lane == 1) v.stats.num_traversed_per_pixel[btg.pixel_id] = EGR_STAMP31(D.bw_t1), v.stats.num_accumulated_per_pixel[btg.pixel_id] = (int32_t)D.bw_rows0;
            })
    }
    if constexpr (TEAM > 1) {
        // no tiles left: this wave takes batches of bounce hits its team mates have queued until all of them are through
        if (lane == 0) atomicAdd(&bteam.done, 1u);
        records += bwd_team_help<TEAM>(v, exp_power, bteam, gt_vals_all, W.stage, wv, lane);
    }
    if (lane == 0 && records) atomicAdd(v.control + CW_BUCKET_RECORDS, records);
}
