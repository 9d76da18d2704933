// k_forward_chain: ONE bounce step of ONE tile (R1 ray, R2 traversal + candidate evaluation, R3 compositing, raw step results).
// Included into the task loop of the kernel; expects `step`, `tq`, `tb`, `near_plane`, GRADS, CUBE, BATCH (`bframe`, `bcam`, `last_frame`) and forward_decl.inc.
// A `continue` ends this step of this tile. OBJ (k_forward_objects: `oq`, `oacc`): the primary step composites per-object coverage instead of the appearance
// and writes the query's outputs at the tile's end; it keeps no ray state and touches neither statistic.
        const uint32_t task = tq;
        const TaskGeom tg = task_geom(v, tb, lane); // (tb == tq outside a batch)
        const StateRef S = state_of(v, task, lane);
        const size_t chain_head = (size_t)step * (BATCH ? v.num_tasks * v.batch_frames : v.num_tasks) + task; // (a batch's task index carries the frame: its tables hold tasks x frames per step)
        if (GRADS && lane == 0) v.task_last_block[chain_head] = 0xFFFFFFFFu; // nothing recorded yet
        if constexpr (OBJ) { // (k_forward_objects) this lane's coverage sums start at +0: oacc[j][lane], a column per lane that no other lane touches
            for (uint32_t j = 0; j < oq.num_bits; j++) oacc[j * EGR_WAVE + (uint32_t)lane] = 0.0f;
        }

        // ---- R1: ray for this step ----------------------------------------------------------------------
        bool active = tg.inside;
        f3 ro = mk3(0, 0, 0), rd = mk3(0, 0, 1);
        uint32_t seed = 0;
        if (step == 0) {
            if (active) {
                if constexpr (BATCH) { // frame f of a batch: the f-th of the sequential launches would see total_num_calls + f + 1 (its prologue adds 1)
                    seed = tea4(tg.pixel_id, (uint32_t)*v.meta.total_num_calls + bframe + 1u);
                    ro = mk3(bcam[0], bcam[1], bcam[2]);
                    rd = primary_direction(v, tg.px, tg.py, *v.cfg.jitter_primary_rays != 0, seed, bcam[12], bcam + 3);
                } else {
                    seed = tea4(tg.pixel_id, (uint32_t)*v.meta.total_num_calls); // shaders.cu:88
                    ro = mk3(v.cam.origin[0], v.cam.origin[1], v.cam.origin[2]);
                    rd = primary_direction(v, tg.px, tg.py, *v.cfg.jitter_primary_rays != 0, seed, tanf(*v.cam.vertical_fov_radians / 2.0f), v.cam.rotation_w2c);
                }
            }
        } else {
            active = active && S.ld(F_ALIVE) != 0.0f;
            if (active) {
                ro = S.ld3(F_RAY_O);
                rd = S.ld3(F_RAY_D);
                seed = f2u(S.ld(F_SEED));
            }
        }
        if (__ballot(active) == 0ull) continue;

        EGR_STATS(const unsigned long long tm0 = __builtin_amdgcn_s_memtime();)
        EGR_TIMES(const unsigned long long tt0 = __builtin_amdgcn_s_memrealtime(); uint32_t tt_batches = 0u, tt_evals = 0u, tt_offers = 0u, tt_tall = 0u; unsigned long long tt_wait = 0ull;)
        // ---- R2: traversal + candidate evaluation (shaders.cu:9-75) -------------------------------------
        // Primary tiles: ONE frustum per tile - the walk collects the leaves the tile's pyramid meets, then every lane tests its own ray against
        // them, one leaf after the other (records through the scalar cache). Bounce tiles: PAIRS - the walk queues (ray, leaf) pairs in LDS,
        // the candidate test runs on batches of 64 pairs, one lane each (a "find a leaf, wait for the wave, evaluate" loop per ray pays
        // max-over-lanes of every leaf search: measured 18 % / 11 % SIMT efficiency on primary / bounce rays in round 1).
        const bool ray_ok = active && v.num_nodes != 0u && finite3(ro) && finite3(rd); // NaN rays (ggx_brdf.h:163) hit nothing; no gaussians: no tree
        const unsigned long long act_mask = __ballot(ray_ok);
        // the ray in the quantisation frame of the tree: cell = (x - o) * s + 2, same t parametrisation.
        // slab plane distance t = (cell - oq) / (d * s) is evaluated as fma(cell, invq, -oq * invq).
        // A direction component of exactly 0 (one primary ray in about 3e7 has one: a cancellation to the last bit) would make both
        // plane distances of that axis inf - inf = NaN and DROP the axis from the slab test: still conservative, but that ray then
        // overlaps every box along its line whatever their position on the dropped axis, and a packet walks what any of its rays
        // overlaps - one such tile took 12 ms, three times the rest of the launch (one launch in twenty of the bench had one). The
        // pruning test therefore sees a tiny component instead: the planes land at -+1e25 and the axis decides by the origin alone.
        auto nz = [](float x) { return fabsf(x) < 1e-30f ? copysignf(1e-30f, x) : x; };
        const f3 invq = mk3(1.0f / (nz(rd.x) * v.frame.sx), 1.0f / (nz(rd.y) * v.frame.sy), 1.0f / (nz(rd.z) * v.frame.sz));
        const f3 ncq = mk3(-((ro.x - v.frame.ox) * v.frame.sx + 2.0f) * invq.x, -((ro.y - v.frame.oy) * v.frame.sy + 2.0f) * invq.y,
                           -((ro.z - v.frame.oz) * v.frame.sz + 2.0f) * invq.z);
        uint32_t cnt = 0, traversed = 0;
        const bool vals_il = step == 0 && v.rays_per_task == (uint32_t)EGR_WAVE; // (= `packet` below: the layout of this step's (alpha, record) lists, forward_decl.inc)
        uint32_t ext = EGR_EXT_NONE; // this ray's extension block (lists longer than cand_cap)
        auto ext_alloc = [&]() -> uint32_t { // one lane: take an extension block; EGR_EXT_NONE - 1 = none left
            const uint32_t e = atomicAdd(v.control + CW_EXT_BUMP, 1u);
            return e < v.ext_blocks_cap ? e : EGR_EXT_NONE - 1u;
        };
        // Total transmittance (shaders.cu:70, Q1): the product of (1 - alpha) over ALL accepted candidates. The reference multiplies in the order of its
        // list and rounds every partial product to fp32, so its last bits depend on an order that is unspecified upstream; here the factors (exact in
        // fp64) are multiplied in fp64 and rounded ONCE: within n / 2 fp32 ulps of what any order gives upstream, and the same whatever order this
        // implementation's list has - a ray's list order (task shape, team help) no longer shows in any output.
        double full_Td = 1.0;
        float full_T = 1.0f;
        bool overflow = false;
        EGR_STATS(uint32_t st_visits = 0, st_leafhits = 0, st_inner = 0, st_outer = 0, st_batches = 0u; unsigned long long st_eval_cycles = 0ull, st_batch_cycles = 0ull;)
        int seg = 0;                 // which of the three walked segments is active (see the walk below)
        float seg_lo, seg_hi;
        auto evaluate = [&](uint32_t prim, const float4 &w0, const float4 &w1, const float4 &w2, auto a2src, const f3 &lo_pre) {
            float t = 0.0f, alpha = 0.0f;
            const int r = test_candidate<CUBE, false>(fc, step, seg, near_plane, ro, rd, prim, w0, w1, w2, a2src, t, alpha, &lo_pre);
            if (r == 0 || r == 3) return;
            traversed++;
            if (r == 1) return;
            full_Td *= 1.0 - (double)alpha; // :70
            if (cnt < v.cand_cap) {
                keys[EGR_KEY_AT(lane, cnt)] = t;
                vals[EGR_VAL_AT(lane, cnt)] = make_float2(alpha, u2f(prim));
                cnt++;
            } else {
                if (ext == EGR_EXT_NONE) ext = ext_alloc();
                const uint32_t e = cnt - v.cand_cap;
                if (ext < EGR_EXT_NONE - 1u && e < EGR_EXT_BLOCK) {
                    v.ext_keys[(size_t)ext * EGR_EXT_BLOCK + e] = t;
                    v.ext_vals[(size_t)ext * EGR_EXT_BLOCK + e] = make_float2(alpha, u2f(prim));
                    cnt++;
                } else {
                    overflow = true;
                }
            }
        };
        // Coherence decides HOW the tree is walked. Primary tiles (coherent: all rays leave the camera origin) walk it as ONE frustum: the
        // node test is per tile, leaf records come through the scalar cache (one request per wave instead of 64 divergent gathers) and every
        // lane tests its own ray against them. Bounce tiles of real scenes are incoherent even at 4-pixel scale (measured union 2.1x for 4
        // lanes, 4.7x for 64; a packet walk chosen by measured coherence never paid, profiles/HISTORY.md) and walk as (ray, node) pairs.
        const bool packet = step == 0 && v.rays_per_task == (uint32_t)EGR_WAVE; // (small tasks: a packet would leave most lanes idle)
        // The tree bounds each gaussian's ELLIPSOID (image of the unit sphere), not its cube: an accepted hit's response
        // point lies inside the ellipsoid (|u|^2 <= 1, shaders.cu:48), so walking a segment finds every accepted hit whose
        // response point lies on that segment, with far fewer false-positive record fetches than cube boxes (the walk is
        // bound by random cache-line fetches). The reference also accepts hits whose response point lies OUTSIDE
        // [tmin,tmax] as long as the cube overlaps the segment (quirk Q1): those are exactly the hits found by walking
        // [0,tmin) and (tmax,inf) and keeping the ones whose cube still overlaps [tmin,tmax] (the cube test below always
        // uses the launch's near/far planes). Three disjoint ownership ranges -> every accepted candidate counted once.
        const bool by_pairs = !packet;
        if (by_pairs) { // publish the rays; per-ray results accumulate in LDS over the three segments
            rayp[lane][0] = make_float4(ro.x, ro.y, ro.z, rd.x), rayp[lane][1] = make_float4(rd.y, rd.z, invq.x, invq.y), rayp[lane][2] = make_float4(invq.z, ncq.x, ncq.y, ncq.z);
            gcnt[lane] = 0u, gtrav[lane] = 0u, gext[lane] = EGR_EXT_NONE;
        }
        // Segment 2 (t > far) can only hold candidates if some box lies farther than the far plane: with every box inside the
        // build frame (no sentinels) that needs a frame corner farther than `far` from the ray origin.
        bool beyond_far_empty = false;
        if (!sentinels) {
            const float fx0 = v.frame.ox - 2.0f / v.frame.sx, fx1 = v.frame.ox + 65534.0f / v.frame.sx;
            const float fy0 = v.frame.oy - 2.0f / v.frame.sy, fy1 = v.frame.oy + 65534.0f / v.frame.sy;
            const float fz0 = v.frame.oz - 2.0f / v.frame.sz, fz1 = v.frame.oz + 65534.0f / v.frame.sz;
            const float dx = fmaxf(fabsf(ro.x - fx0), fabsf(ro.x - fx1)), dy = fmaxf(fabsf(ro.y - fy0), fabsf(ro.y - fy1)),
                        dz = fmaxf(fabsf(ro.z - fz0), fabsf(ro.z - fz1));
            const bool reaches = !(dx * dx + dy * dy + dz * dz < far_plane * far_plane * 0.999f); // NaN-safe: unknown counts as "reaches"
            beyond_far_empty = __ballot(ray_ok && reaches) == 0ull;
        }
        const float near_c = near_plane, far_c = far_plane;
        seg_lo = near_c, seg_hi = far_c;
        for (seg = 0; seg < (CUBE ? 1 : 3); seg++) {
            if (seg == 1) {
                if (!(near_plane > 0.0f)) continue; // bounce steps start at 0: nothing before the segment
                seg_lo = 0.0f, seg_hi = near_c;
            } else if (seg == 2) {
                if (beyond_far_empty) continue; // no box reaches past the far plane for any ray of this tile
                seg_lo = far_c, seg_hi = 3.0e38f;
            }
        if (packet) {
            // ---- frustum walk (primary tiles). All 64 rays leave ONE point (core/camera.h:17-36: the camera origin), so the tile is a thin
            // pyramid: bundle axis e_w, lateral ranges u in [umin, umax], v in [vmin, vmax] of the ray directions (computed from the
            // rays themselves: jitter and all). A node is entered when its BOX meets the pyramid between the segment's two distances - one
            // interval test per child slot for the whole tile (about 50 fast VALU instructions for EIGHT nodes x 8 slots, one lane
            // each) where the packet walk of rounds 1-3 had every lane test its own ray against every slot of one node (8 x 31
            // instructions per node, one dependent scalar-cache round trip per node). The walk pops up to eight nodes per iteration
            // from a wave-wide LDS stack, inner hits go back onto it, leaf hits into the leaf buffer; the buffered leaves are then
            // evaluated by ONE instance of the candidate test, every lane for its own ray and only against the leaves its ray can meet (a
            // per-ray sphere pre-test, records staged in LDS: below; exact statistics: every leaf, records through the scalar cache, the
            // next leaf's record requested before the current one is worked off). The test is conservative (interval
            // arithmetic on the box's projections + half a cell of slack): it may enter a box no ray hits, never the reverse.
            const unsigned long long okm = __ballot(ray_ok);
            if (okm != 0ull) {
                auto wsum = [](float x) {
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
                    return x;
                };
                auto wmin = [](float x) {
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) x = fminf(x, __shfl_xor(x, off));
                    return x;
                };
                auto wmax = [](float x) {
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) x = fmaxf(x, __shfl_xor(x, off));
                    return x;
                };
                auto uni = [](float x) { return u2f((uint32_t)__builtin_amdgcn_readfirstlane((int)f2u(x))); };
                const f3 dz = ray_ok ? rd : mk3(0, 0, 0);
                const f3 ew = normalize(mk3(wsum(dz.x), wsum(dz.y), wsum(dz.z)));
                const f3 eu = normalize(cross(fabsf(ew.z) < 0.9f ? mk3(0, 0, 1) : mk3(1, 0, 0), ew)), ev = cross(ew, eu);
                const float pw = dot(rd, ew), pu = dot(rd, eu) / pw, pv = dot(rd, ev) / pw;
                // (a bundle that is not narrow - no 8x8 tile of a pinhole camera is - or a degenerate axis: no lateral culling)
                const bool narrow = wmin(ray_ok ? pw : 1.0f) > 0.5f && isfinite(ew.x + ew.y + ew.z);
                const float big = 3.0e38f, lat = 4e-6f; // lateral slack: directions are unit vectors to ~1e-7
                const float umin = narrow ? fminf(wmin(ray_ok ? pu : big) - lat, -lat) : -big, umax = narrow ? fmaxf(wmax(ray_ok ? pu : -big) + lat, lat) : big;
                const float vmin = narrow ? fminf(wmin(ray_ok ? pv : big) - lat, -lat) : -big, vmax = narrow ? fmaxf(wmax(ray_ok ? pv : -big) + lat, lat) : big;
                const float kappa = narrow ? wmax(ray_ok ? 1.0f / pw : 1.0f) * 1.000001f : big; // distance along a ray <= kappa x (distance along the axis)
                // everything below in the tree's cell coordinates: world offset = (cell - oq) / scale per axis
                const float isx = 1.0f / v.frame.sx, isy = 1.0f / v.frame.sy, isz = 1.0f / v.frame.sz;
                const f3 cam_o = BATCH ? mk3(bcam[0], bcam[1], bcam[2]) : mk3(v.cam.origin[0], v.cam.origin[1], v.cam.origin[2]); // the rays' common origin (NOT this lane's `ro`: a lane without a ray - a masked pixel - holds none, and lane 0's value is what `uni` broadcasts)
                const float oqx = (cam_o.x - v.frame.ox) * v.frame.sx + 2.0f, oqy = (cam_o.y - v.frame.oy) * v.frame.sy + 2.0f, oqz = (cam_o.z - v.frame.oz) * v.frame.sz + 2.0f;
                // half projections: X(box) in [S1 - S2, S1 + S2], S1 = sum_a (e_a / 2s_a) (lo_a + hi_a) - C, S2 = sum_a |e_a / 2s_a| (hi_a - lo_a)
                const float hux = uni(0.5f * eu.x * isx), huy = uni(0.5f * eu.y * isy), huz = uni(0.5f * eu.z * isz);
                const float hvx = uni(0.5f * ev.x * isx), hvy = uni(0.5f * ev.y * isy), hvz = uni(0.5f * ev.z * isz);
                const float hwx = uni(0.5f * ew.x * isx), hwy = uni(0.5f * ew.y * isy), hwz = uni(0.5f * ew.z * isz);
                const float cu = uni(2.0f * (hux * oqx + huy * oqy + huz * oqz)), cv = uni(2.0f * (hvx * oqx + hvy * oqy + hvz * oqz)), cw = uni(2.0f * (hwx * oqx + hwy * oqy + hwz * oqz));
                const float slack = uni(isx + isy + isz); // one cell diagonal, world units (the boxes carry a full extra cell each side on top)
                const float f_umin = uni(umin), f_umax = uni(umax), f_vmin = uni(vmin), f_vmax = uni(vmax), f_kappa = uni(kappa);
                const float f_lo = uni(seg_lo), f_hi = uni(seg_hi);
                const bool narrow_u = __builtin_amdgcn_readfirstlane(narrow ? 1 : 0) != 0;
                auto frustum_hit = [&](const uint4 &q) -> bool {
                    const float lx = (float)(q.x & 0xFFFFu), ly = (float)(q.x >> 16), lz = (float)(q.y & 0xFFFFu);
                    const float hx = (float)(q.y >> 16), hy = (float)(q.z & 0xFFFFu), hz = (float)(q.z >> 16);
                    const float cx = lx + hx, cy = ly + hy, cz = lz + hz, ex = hx - lx, ey = hy - ly, ez = hz - lz;
                    const float u1 = fmaf(hux, cx, fmaf(huy, cy, fmaf(huz, cz, -cu))), u2 = fmaf(fabsf(hux), ex, fmaf(fabsf(huy), ey, fabsf(huz) * ez));
                    const float v1 = fmaf(hvx, cx, fmaf(hvy, cy, fmaf(hvz, cz, -cv))), v2 = fmaf(fabsf(hvx), ex, fmaf(fabsf(hvy), ey, fabsf(hvz) * ez));
                    const float w1 = fmaf(hwx, cx, fmaf(hwy, cy, fmaf(hwz, cz, -cw))), w2 = fmaf(fabsf(hwx), ex, fmaf(fabsf(hwy), ey, fabsf(hwz) * ez));
                    const float wmx = w1 + w2 + slack, wmn = w1 - w2 - slack; // the box's extent along the axis
                    // inside the pyramid: w > 0, umin w <= u <= umax w, vmin w <= v <= vmax w (umin, vmin < 0 < umax, vmax); distance in [lo, hi]
                    bool keep = wmx > 0.0f;
                    if (!narrow_u) return true;
                    keep &= fmaf(-f_umin, wmx, u1 + u2) >= -slack; // max over the box of (u - umin w)
                    keep &= fmaf(f_umax, wmx, u2 - u1) >= -slack;  // max of (umax w - u)
                    keep &= fmaf(-f_vmin, wmx, v1 + v2) >= -slack;
                    keep &= fmaf(f_vmax, wmx, v2 - v1) >= -slack;
                    keep &= wmx * f_kappa >= f_lo;
                    keep &= wmn <= f_hi;
                    if (sentinels) keep |= ((q.x & 0xFFFFu) == 0u) | ((q.x >> 16) == 0u) | ((q.y & 0xFFFFu) == 0u) | ((q.y >> 16) == 65535u) | ((q.z & 0xFFFFu) == 65535u) | ((q.z >> 16) == 65535u); // a box that left the build frame: no culling
                    return keep;
                };
                // lengths of the side planes' normals (1, 0, -umax) ... in the (e_u, e_v, e_w) frame
                const float n_umin = sqrtf(fmaf(f_umin, f_umin, 1.0f)), n_umax = sqrtf(fmaf(f_umax, f_umax, 1.0f)), n_vmin = sqrtf(fmaf(f_vmin, f_vmin, 1.0f)), n_vmax = sqrtf(fmaf(f_vmax, f_vmax, 1.0f));
                const uint32_t m = (uint32_t)lane & 7u, grp = (uint32_t)lane >> 3;
                uint32_t *__restrict__ ugstk = v.stack_spill + (size_t)slot * EGR_GSTK * EGR_WAVE; // pending subtrees beyond the LDS part (deep trees; agent-scope accesses)
                constexpr uint32_t UGSTK_CAP = (uint32_t)EGR_GSTK * EGR_WAVE;
                bool f_over = false;
                uint32_t top = 1u, nl = 0u; // wave-uniform heights of the node stack and of the leaf buffer
                if (lane == 0) pstk[0] = 0u;
                wave_sync();
                for (;;) {
                    const bool do_eval = nl >= (uint32_t)EGR_WAVE || (top == 0u && nl > 0u);
                    if (!do_eval && top == 0u) break;
                    if (do_eval) {
                        EGR_STATS(const unsigned long long te0 = __builtin_amdgcn_s_memtime();)
                        // First the leaves themselves, ONE LANE PER LEAF: a gaussian's box is a loose bound of a rotated ellipsoid (up to 1.7 radii
                        // along a pyramid side's normal, plus the cells of the quantisation), and every leaf that reaches the loop below costs the
                        // whole candidate test in all 64 lanes. The leaf's bounding SPHERE (bvh.hip: centre, squared radius) is tested against the
                        // four side planes of the tile's pyramid - one 16-B fetch and ~ 25 instructions for 64 leaves - and the survivors are
                        // compacted in place. Conservative: an accepted candidate's response point lies inside the ellipsoid, hence inside the
                        // sphere, and on one of the tile's rays, hence inside the pyramid.
                        if (narrow_u) {
                            EGR_STATS(const unsigned long long tf0 = __builtin_amdgcn_s_memtime(); st_batches += nl;)
                            uint32_t nk = 0u;
                            for (uint32_t base = 0u; base < nl; base += (uint32_t)EGR_WAVE) {
                                const uint32_t nb = min(nl - base, (uint32_t)EGR_WAVE);
                                const uint32_t leaf = lbuf[base + min((uint32_t)lane, nb - 1u)];
                                const float4 sp = v.bsph[leaf];
                                const f3 a = mk3(sp.x - cam_o.x, sp.y - cam_o.y, sp.z - cam_o.z);
                                const float au = dot(a, eu), av = dot(a, ev), aw = dot(a, ew);
                                // radius: padded by k_instances for the rounding of the centre, + 0.5 % + the rounding of the three projections
                                const float rad = sqrtf(fmaxf(sp.w, 0.0f)) * 1.005f + 2e-6f * (fabsf(a.x) + fabsf(a.y) + fabsf(a.z));
                                bool keep = (uint32_t)lane < nb && sp.w >= 0.0f;
                                keep = keep && !(fmaf(f_umin, aw, -au) > rad * n_umin) && !(fmaf(-f_umax, aw, au) > rad * n_umax); // outside a side plane by more than the radius
                                keep = keep && !(fmaf(f_vmin, aw, -av) > rad * n_vmin) && !(fmaf(-f_vmax, aw, av) > rad * n_vmax);
                                wave_sync(); // every lane has read its leaf: the compacted list overwrites the buffer from its start
                                const unsigned long long km = __builtin_amdgcn_ballot_w64(keep);
                                if (keep) lbuf[nk + __builtin_amdgcn_mbcnt_hi((uint32_t)(km >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)km, 0u))] = leaf;
                                nk += (uint32_t)__popcll(km);
                                wave_sync();
                            }
                            nl = nk;
                            EGR_STATS(st_batch_cycles += __builtin_amdgcn_s_memtime() - tf0;)
                        }
                        EGR_TIMES_IS(9, chain_leaves += nl;) // (the leaves this tile's primary step evaluates - is it a predictor of the chain's duration?)
                        if (nl != 0u) {
                        // ONE instance of the candidate test for every leaf (not one per unrolled slot): bit-identical gaussians then get
                        // bit-identical distances wherever they sit - an ulp between two copies of a duplicated object decides what the
                        // tie rule of forward_pass.cu:62 drops. The next leaf's record is requested before this one is worked off.
                        // All rays of the tile leave the camera origin, so a leaf's object-space ORIGIN W o + w is one vector for the whole tile: one
                        // lane per leaf computes it (the expression every other caller of the candidate test evaluates per ray: object_origin) and
                        // the loop below reads it back with one broadcast LDS read instead of twelve VALU instructions in every lane. The ray table is
                        // free during a primary step (only pair walks publish rays) and holds the 192 vectors a round can have.
                        static_assert(EGR_WAVE + 8 * EGR_FPOP * EGR_WIDTH <= 3 * EGR_WAVE, "the ray table holds one float4 per buffered leaf");
                        static_assert(3 * EGR_WAVE + 5 * EGR_WAVE <= EGR_LBUF, "the leaf buffer holds five more words per leaf of a 64-leaf chunk behind its 192 leaf indices");
                        if constexpr (CUBE) { // exact statistics count an `outside` pair (test_candidate returns 1): every lane tests every buffered leaf
                        float4 *const llo = &rayp[0][0];
                        for (uint32_t base = 0u; base < nl; base += (uint32_t)EGR_WAVE) {
                            const uint32_t li = base + (uint32_t)lane;
                            if (li < nl) {
                                const uint32_t leaf = lbuf[li];
                                const float4 g0 = v.inst_w[4 * (size_t)leaf], g1 = v.inst_w[4 * (size_t)leaf + 1], g2 = v.inst_w[4 * (size_t)leaf + 2];
                                const f3 lo_ = object_origin(g0, g1, g2, cam_o);
                                llo[li] = make_float4(lo_.x, lo_.y, lo_.z, 0.0f);
                            }
                        }
                        wave_sync();
                        uint32_t pn = (uint32_t)__builtin_amdgcn_readfirstlane((int)lbuf[0]);
                        float4 n0 = load_f4_uniform(v.inst_w, 4 * pn), n1 = load_f4_uniform(v.inst_w, 4 * pn + 1), n2 = load_f4_uniform(v.inst_w, 4 * pn + 2), n3 = load_f4_uniform(v.inst_w, 4 * pn + 3);
                        uint32_t pn_next = lbuf[min(1u, nl - 1u)];
                        float4 nlo = llo[0];
#pragma unroll 1
                        for (uint32_t i = 0; i < nl; i++) {
                            const uint32_t p = pn;
                            const float4 w0 = n0, w1 = n1, w2 = n2, a2 = n3;
                            const f3 lo_pre = mk3(nlo.x, nlo.y, nlo.z);
                            pn = (uint32_t)__builtin_amdgcn_readfirstlane((int)pn_next); // (the index was read from LDS an iteration ago: no LDS round trip in front of the record request)
                            pn_next = lbuf[min(i + 2u, nl - 1u)];
                            n0 = load_f4_uniform(v.inst_w, 4 * pn), n1 = load_f4_uniform(v.inst_w, 4 * pn + 1), n2 = load_f4_uniform(v.inst_w, 4 * pn + 2), n3 = load_f4_uniform(v.inst_w, 4 * pn + 3);
                            nlo = llo[min(i + 1u, nl - 1u)];
                            EGR_STATS(st_leafhits += ray_ok ? 1u : 0u, st_outer += (lane == 0);)
                            if (ray_ok) evaluate(p, w0, w1, w2, a2, lo_pre);
#if defined(__HIP_DEVICE_COMPILE__)
                            // (the NEXT record is in flight during the test above. Its unused dwords - the W rows' fourth components, half of the live
                            // quarter - stay allocated until here: the compiler otherwise hands those destination registers to the body, e.g. for the saved
                            // exec mask, and has to wait for the whole load before the body's first instruction - the prefetch hid nothing)
                            asm volatile("" ::"s"(n0.w), "s"(n1.w), "s"(n2.w), "s"(n3.x), "s"(n3.y));
#endif
                        }
                        } else {
                        // Default launches: a pair whose response point lies outside the ellipsoid returns 0 or 3 - never counted, never appended - and with
                        // gaussians about two tiles across three quarters of a tile's (ray, leaf) pairs are just that, found out only after most of
                        // candidate_geometry_from, in every lane, for every leaf. So, in chunks of 64 buffered leaves and lane = ray throughout:
                        // 0. STAGING, one lane per leaf: what the candidate test reads of the leaf's record (rows of W, opacity, sigma factor), the
                        //    object-space origin (see above) and the padded sphere go to LDS - the ray table holds the rows with the origin in their
                        //    fourth components, the leaf buffer behind its 192 indices the other five words. The records are fetched ONCE per tile,
                        //    coalesced by leaf; a gather per lane from global memory in the loop of step 2 made an iteration 2.6 times as expensive
                        //    as the scalar fetch it replaced and the kernel slower (profiles/HISTORY.md, profiles/r19/).
                        // 1. the PRE-TEST (trace.hip: ray_misses_sphere): every leaf of the chunk in turn, wave-uniform, its sphere read with a broadcast
                        //    LDS read, a dozen VALU instructions; a lane keeps bit i of a two-dword mask for every leaf its ray can meet. A rejected
                        //    pair is one the candidate test would have returned 0 or 3 for.
                        // 2. the SURVIVOR LOOP: every lane walks ITS OWN kept leaves in ascending buffer order - the order it met them in when every
                        //    lane tested every leaf, so its list, its counters and the factors of full_Td come out entry for entry as they did - and
                        //    different lanes work on different leaves in one iteration: the loop runs for the longest mask of any lane, not for the
                        //    number of leaves (per chunk: a mask over the whole round would need the round's records in LDS, 10.7 KB per wave). A lane
                        //    reads its record from LDS by slot; the next slot is taken off the mask and its reads are under way while the current
                        //    record is worked off. Still ONE instance of the candidate test (see above).
                        constexpr int NW = EGR_WAVE / 32;
                        uint32_t *const lx = lbuf + 3 * EGR_WAVE; // five words per leaf of the chunk: opacity, sigma factor, a / rad
                        const float rd2 = dot(rd, rd);
                        for (uint32_t cbase = 0u; cbase < nl; cbase += (uint32_t)EGR_WAVE) {
                        const uint32_t cn = min(nl - cbase, (uint32_t)EGR_WAVE);
                        if ((uint32_t)lane < cn) { // STAGING, one lane per leaf of the chunk: the record as the candidate test reads it, the object-space origin, the sphere
                            const uint32_t leaf = lbuf[cbase + (uint32_t)lane];
                            const float4 g0 = v.inst_w[4 * (size_t)leaf], g1 = v.inst_w[4 * (size_t)leaf + 1], g2 = v.inst_w[4 * (size_t)leaf + 2], g3 = v.inst_w[4 * (size_t)leaf + 3];
                            const f3 lo_ = object_origin(g0, g1, g2, cam_o);
                            const f3 an = staged_sphere(v.bsph[leaf], g0, g1, g2, lo_, cam_o);
                            rayp[lane][0] = make_float4(g0.x, g0.y, g0.z, lo_.x), rayp[lane][1] = make_float4(g1.x, g1.y, g1.z, lo_.y), rayp[lane][2] = make_float4(g2.x, g2.y, g2.z, lo_.z);
                            lx[5 * lane] = f2u(g3.z), lx[5 * lane + 1] = f2u(g3.w), lx[5 * lane + 2] = f2u(an.x), lx[5 * lane + 3] = f2u(an.y), lx[5 * lane + 4] = f2u(an.z);
                        }
                        wave_sync();
                        uint32_t mk[NW]; // (indexed by unrolled constants only: a dynamic index would send it to scratch)
#pragma unroll
                        for (int w = 0; w < NW; w++) {
                            uint32_t m = 0u;
                            if (32u * (uint32_t)w < cn) {
                                const uint32_t nb = min(cn - 32u * (uint32_t)w, 32u);
#pragma unroll 4 // (four leaves' LDS reads in flight)
                                for (uint32_t j = 0; j < nb; j++) {
                                    const uint32_t i = 32u * (uint32_t)w + j;
                                    const f3 an = mk3(u2f(lx[5u * i + 2u]), u2f(lx[5u * i + 3u]), u2f(lx[5u * i + 4u]));
                                    m |= (ray_misses_sphere(an, rd, rd2) ? 0u : 1u) << j;
                                }
                            }
                            mk[w] = ray_ok ? m : 0u;
                        }
                        constexpr uint32_t NO_SLOT = 0xFFFFFFFFu;
                        auto pop = [&]() -> uint32_t { // this lane's lowest kept slot, taken off its mask (selects, no indexing); NO_SLOT when none is left
                            uint32_t word = 0u, base = 0u;
#pragma unroll
                            for (int w = NW - 1; w >= 0; w--) {
                                const bool h = mk[w] != 0u;
                                word = h ? mk[w] : word, base = h ? 32u * (uint32_t)w : base;
                            }
                            const uint32_t rest = word & (word - 1u);
#pragma unroll
                            for (int w = 0; w < NW; w++) mk[w] = base == 32u * (uint32_t)w ? rest : mk[w]; // (no word left: base 0, and word 0 stays 0)
                            return base + (uint32_t)__ffs((int)word) - 1u;                                    // (no word left: 0 + 0 - 1 = NO_SLOT)
                        };
                        uint32_t s_n = pop(); // the slot worked off next; a lane without one parks on the chunk's last slot and idles
                        uint32_t sc = min(s_n, cn - 1u);
                        uint32_t leaf_n = lbuf[cbase + sc];
                        float4 n0 = rayp[sc][0], n1 = rayp[sc][1], n2 = rayp[sc][2]; // (rows of W, the origin in their fourth components)
                        float q0 = u2f(lx[5u * sc]), q1 = u2f(lx[5u * sc + 1u]);
#pragma unroll 1
                        while (__ballot(s_n != NO_SLOT) != 0ull) {
                            const bool have = s_n != NO_SLOT;
                            const uint32_t p = leaf_n;
                            const float4 w0 = n0, w1 = n1, w2 = n2, a2 = make_float4(0.0f, 0.0f, q0, q1); // (opacity, sigma factor: what the candidate test reads of the live quarter)
                            const f3 lo_pre = mk3(n0.w, n1.w, n2.w);
                            s_n = pop(), sc = min(s_n, cn - 1u); // the next record's LDS reads are under way during the test below
                            leaf_n = lbuf[cbase + sc];
                            n0 = rayp[sc][0], n1 = rayp[sc][1], n2 = rayp[sc][2];
                            q0 = u2f(lx[5u * sc]), q1 = u2f(lx[5u * sc + 1u]);
                            EGR_STATS(st_leafhits += have ? 1u : 0u, st_outer += (lane == 0);)
                            if (have) evaluate(p, w0, w1, w2, a2, lo_pre);
                        }
                        wave_sync(); // every lane has read its last record: the next chunk's staging overwrites them
                        }
                        }
                        }
                        nl = 0u;
                        wave_sync(); // the buffer is refilled below
                        EGR_STATS(st_eval_cycles += __builtin_amdgcn_s_memtime() - te0;)
                        if (top == 0u) break;
                    }
                    // (EGR_FPOP x 8 nodes per iteration: lane group g takes the g-th, (g + 8)-th ... node from the top; their lines are requested together)
                    const uint32_t npop = min(top, 8u * (uint32_t)EGR_FPOP);
                    uint4 sl_[EGR_FPOP];
#pragma unroll
                    for (int u = 0; u < EGR_FPOP; u++) {
                        const uint32_t gi = grp + 8u * (uint32_t)u;
                        const uint32_t e = top - 1u - min(gi, top - 1u);
                        uint32_t node = pstk[min(e, (uint32_t)EGR_PSTK - 1u)];
                        if (top > (uint32_t)EGR_PSTK && e >= (uint32_t)EGR_PSTK) node = __hip_atomic_load(ugstk + (e - EGR_PSTK), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // (rare)
                        sl_[u] = wnodes[(size_t)node * EGR_WIDTH + m]; // (a group beyond the popped nodes re-reads the bottom node and is turned into an empty slot)
                        if (!(gi < npop)) sl_[u].w = EGR_EMPTY_SLOT;
                        EGR_STATS(st_visits += (m == 0u && gi < npop) ? 1u : 0u;)
                    }
                    top -= npop;
                    EGR_STATS(st_inner += (lane == 0);)
                    wave_sync(); // the stack reads above come before the pushes below
#pragma unroll
                    for (int u = 0; u < EGR_FPOP; u++) {
                        const uint4 sl = sl_[u];
                        const bool hit = frustum_hit(sl) & (sl.w != EGR_EMPTY_SLOT);
                        const bool leaf = (int)sl.w < 0;
                        const unsigned long long hm = __builtin_amdgcn_ballot_w64(hit), lm = __builtin_amdgcn_ballot_w64(leaf);
                        const unsigned long long im = hm & ~lm, fm = hm & lm;
                        const uint32_t at = top + __builtin_amdgcn_mbcnt_hi((uint32_t)(im >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)im, 0u));
                        if (hit & !leaf) {
                            if (at < (uint32_t)EGR_PSTK) pstk[at] = sl.w;
                            else if (at - EGR_PSTK < UGSTK_CAP) __hip_atomic_store(ugstk + (at - EGR_PSTK), sl.w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            else f_over = true; // more pending subtrees than LDS + the spill column hold: flagged, not silent
                        }
                        top = min(top + (uint32_t)__popcll(im), (uint32_t)EGR_PSTK + UGSTK_CAP);
                        if (hit & leaf) lbuf[nl + __builtin_amdgcn_mbcnt_hi((uint32_t)(fm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)fm, 0u))] = sl.w & ~EGR_LEAF_FLAG;
                        nl += (uint32_t)__popcll(fm);
                    }
                    wave_sync();
                }
                if (__ballot(f_over) != 0ull) overflow = true;
            }
        } else {
            // ---- pair walk (trace.hip: pair_walk). The rays were published above; the stack starts with one (ray, root) pair per ray.
            const size_t scratch0 = (size_t)slot * EGR_WAVE;
            uint32_t *__restrict__ gstk = v.stack_spill + (size_t)slot * EGR_GSTK * EGR_WAVE; // pair-stack entries beyond the LDS part
            bool g_over = false;
            const uint32_t top = (uint32_t)__popcll(act_mask);
            if ((act_mask >> lane) & 1ull) pstk[__popcll(act_mask & ((1ull << lane) - 1ull))] = (uint32_t)lane << 26; // (ray, root)
            if constexpr (TEAM > 1) { // what a helper needs to know about this walk (no helper is at work: the previous walk waited for that; its last offer may still be on its way out)
                while (uniform_u32(lds_peek(&team.box_count[wv])) != 0u) __builtin_amdgcn_s_sleep(1);
                if (lane == 0) lds_poke(&team.ctx[wv][0], (uint32_t)step | ((uint32_t)seg << 8)), lds_poke(&team.ctx[wv][1], f2u(seg_lo)), lds_poke(&team.ctx[wv][2], f2u(seg_hi)), lds_poke(&team.ctx[wv][3], f2u(near_plane)), lds_poke(&team.ctx[wv][4], (uint32_t)wv);
            }
            wave_sync();
            WalkStats wst;
            // (a third copy for segment 0 without sentinels - nearly every walk of a bounce step: the candidate test then carries no segment dispatch)
            if (!sentinels && seg == 0) pair_walk<false, true, CUBE, TEAM>(v, fc, wsh, wsh, team, wv, scratch0, gstk, step, seg, seg_lo, seg_hi, near_plane, top, g_over, wst);
            else if (sentinels) pair_walk<true, false, CUBE, TEAM>(v, fc, wsh, wsh, team, wv, scratch0, gstk, step, seg, seg_lo, seg_hi, near_plane, top, g_over, wst);
            else pair_walk<false, false, CUBE, TEAM>(v, fc, wsh, wsh, team, wv, scratch0, gstk, step, seg, seg_lo, seg_hi, near_plane, top, g_over, wst);
            EGR_TIMES(tt_batches += wst.inner, tt_evals += wst.outer, tt_offers += wst.offers, tt_tall += wst.tall;)
            EGR_STATS(st_visits += wst.visits, st_leafhits += wst.leafhits, st_inner += wst.inner, st_outer += wst.outer;)
            EGR_STATS(if (lane == 0 && (wst.offers | wst.tall)) atomicAdd(v.control + DG_TEAM_OFFERS, wst.offers), atomicAdd(v.control + DG_TEAM_TALL, wst.tall);)
            if (TEAM > 1 && v.team_help) {
                // pairs of this walk that team mates took: until they are worked off this wave is a helper itself (theirs are the likeliest offers)
                EGR_TIMES(const unsigned long long tw0 = __builtin_amdgcn_s_memrealtime();)
                team_help_while<CUBE, TEAM>(v, fc, wsh_all, team, wv, blockIdx.x * (uint32_t)TEAM, g_over, [&]() { return uniform_u32(lds_peek(&team.busy[wv])) != 0u; });
                EGR_TIMES(tt_wait += __builtin_amdgcn_s_memrealtime() - tw0;)
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); // the helpers' list entries
            }
            if (__ballot(g_over) != 0ull) overflow = true;
        }

        }
        if (by_pairs) { // this lane's ray: what the wave collected for it
            ext = gext[lane], traversed = gtrav[lane];
            cnt = min(gcnt[lane], v.cand_cap + (ext < EGR_EXT_NONE - 1u ? EGR_EXT_BLOCK : 0u));
            if (cnt != gcnt[lane]) overflow = true;
            const uint32_t nbase = min(cnt, v.cand_cap);
            // shaders.cu:70, over ALL accepted candidates (Q1), in list order. Eight (alpha, record) pairs per round trip (the run is
            // padded to a multiple of 8, so the loads stay inside it): one 8-B load per iteration would be one dependent fetch per entry
            for (uint32_t k = 0; k < nbase; k += 8) {
                const float4 a = EGR_VAL_Q(lane, k), b = EGR_VAL_Q(lane, k + 2), c = EGR_VAL_Q(lane, k + 4), d = EGR_VAL_Q(lane, k + 6);
                const float al[8] = {a.x, a.z, b.x, b.z, c.x, c.z, d.x, d.z};
#pragma unroll
                for (int j = 0; j < 8; j++)
                    if (k + (uint32_t)j < nbase) full_Td *= 1.0 - (double)al[j];
            }
            for (uint32_t k = nbase; k < cnt; k++) full_Td *= 1.0 - (double)v.ext_vals[(size_t)ext * EGR_EXT_BLOCK + (k - v.cand_cap)].x;
        }
        full_T = (float)full_Td;
#ifdef EGR_DEBUG_PIXEL // diagnostic build (egr_diag.hpp): the candidate list of one pixel (step 0)
        if (active && step == 0 && tg.pixel_id == (uint32_t)EGR_DEBUG_PIXEL) {
            printf("[pixel %u] cnt %u traversed %u full_T %.9g\n", tg.pixel_id, cnt, traversed, (double)full_T);
            for (uint32_t k = 0; k < cnt && k < v.cand_cap; k++) printf("   k %u t %.9g (%08x) alpha %.9g pos %u gid %u\n", k, (double)keys[EGR_KEY_AT(lane, k)], f2u(keys[EGR_KEY_AT(lane, k)]), (double)vals[EGR_VAL_AT(lane, k)].x, f2u(vals[EGR_VAL_AT(lane, k)].y), v.gid_of_pos[f2u(vals[EGR_VAL_AT(lane, k)].y)]);
        }
#endif
#ifdef EGR_DEBUG_LIST
        if (active && cnt > 0 && cnt <= v.cand_cap) {
            double p = 1.0;
            for (uint32_t k = 0; k < cnt; k++) p *= 1.0 - (double)vals[EGR_VAL_AT(lane, k)].x;
            if (fabs(p - (double)full_T) > 1e-4 * fmax(p, (double)full_T) + 1e-12) {
                printf("[list mismatch] step %d task %u lane %d cnt %u prodlist %.9g full_T %.9g pair walk %d\n", step, task, lane, cnt, p, (double)full_T, (int)by_pairs);
                for (uint32_t k = 0; k < cnt && k < 40; k++) printf("   k %u t %.9g alpha %.9g pos %u\n", k, (double)keys[EGR_KEY_AT(lane, k)], (double)vals[EGR_VAL_AT(lane, k)].x, f2u(vals[k].y));
            }
        }
#endif
        EGR_STATS(const unsigned long long tm1 = __builtin_amdgcn_s_memtime(); {
            const uint32_t cm = wave_max_u32(active ? cnt : 0u); // (primary tiles: the histogram of their longest candidate list)
            const unsigned long long a = wave_sum_u32(st_visits), b = wave_sum_u32(st_leafhits), c2 = wave_sum_u32(st_inner), d = wave_sum_u32(st_outer);
            if (lane == 0 && step == 0) atomicAdd(v.control + DG_LIST_HIST + (cm <= 16u ? 0 : cm <= 24u ? 1 : cm <= 32u ? 2 : cm <= 40u ? 3 : cm <= 48u ? 4 : cm <= 64u ? 5 : 6), 1u);
            if (lane == 0 && st_batches) atomicAdd(diag64(v.control, DG_FILTER_CYC), st_batch_cycles), atomicAdd(diag64(v.control, DG_FILTER_LEAVES), (unsigned long long)st_batches);
            if (lane == 0) atomicAdd(diag64(v.control, DG_LEAF_EVAL_CYC, step > 0), st_eval_cycles), atomicAdd(diag64(v.control, DG_VISITS, step > 0), a), atomicAdd(diag64(v.control, DG_LEAF_HITS, step > 0), b), atomicAdd(diag64(v.control, DG_WALK_ITERS, step > 0), c2), atomicAdd(diag64(v.control, DG_EVAL_ROUNDS, step > 0), d);
        })
        EGR_TIMES(const unsigned long long tt_mid = __builtin_amdgcn_s_memrealtime();) // end of the walk / start of the depth selection
        // ---- R3: depth-ordered compositing (forward_pass.cu:48-137) --------------------------------------
        f3 c_rgb = mk3(0, 0, 0), c_n = mk3(0, 0, 0), c_f0 = mk3(0, 0, 0);
        float c_rough = 0.0f, c_depth = 0.0f, T = 1.0f;
        uint32_t nhits = 0;
        {
            float t_prev = near_plane;    // strict '>' against tmin (forward_pass.cu:62)
            uint32_t k_prev = 0xFFFFFFFFu; // ties: continue in list order after the previous pick
            bool running = active && cnt > 0;
            uint32_t last_block = 0xFFFFFFFFu, cur_block = 0xFFFFFFFFu;
            bool recording = GRADS;
            // Depth order in batches of 8 (= one arena block): ONE scan over the lane's key column keeps the 8 strict
            // successors of (t_prev, k_prev) in (t, k) lexicographic order in registers (sorted insertion, static indices),
            // then the batch is composited front to back. The old "one scan per composited hit" cost Kc+1 passes.
            EGR_STATS(unsigned long long tc_scan = 0ull, tc_alloc = 0ull, tc_av = 0ull, tc_p1 = 0ull, tc_app = 0ull;)
            for (uint32_t it = 0;; it += EGR_HIT_BLOCK_ROWS) {
                EGR_STATS(const unsigned long long tcs0 = __builtin_amdgcn_s_memtime();)
                float kt[8];
                uint32_t ki[8];
#pragma unroll
                for (int j = 0; j < 8; j++) kt[j] = 3.4028235e38f, ki[j] = 0xFFFFFFFFu;
                // Q3 (forward_pass.cu:62): the reference selects in batches of BUFFER_SIZE = 16 with a strict `>` against tmin = the
                // last composited distance, so a hit that ties with the 16th, 32nd, ... composited hit of its ray is dropped. Inside
                // a reference batch (two of these batches of 8) equal distances are all kept, here in list order.
                if ((it & 15u) == 0u) k_prev = 0xFFFFFFFFu;
                if (running) {
                    // Sorted insertion of one key into the eight kept (kt ascending; unused slots hold FLT_MAX): slot j takes its left neighbour if the
                    // key goes in front of that one, the key itself if it goes in front of slot j only, else stays - for the distances that is
                    // med3(key, kt[j-1], kt[j]), ONE instruction per slot; the list indices follow with two selects on the eight compares. A key
                    // that does not qualify enters as FLT_MAX, which is in front of nothing. Strict '<': an equal key stays behind (list order).
                    // (40 instead of the 91 instructions per key the carried-element bubble of rounds 2-3 compiled to; forward chain -2 % dense-init.)
                    auto consider = [&](float tk, uint32_t k) {
                        // (a branch, not selects: scans of long lists - grazing walls, grazing bounce rays - insert next to nothing, and with few lanes left in
                        // a wave whole keys are skipped. Two compares decide it for nearly every key; whether a key that EQUALS the last composited
                        // distance continues the tie - the list-index rule - is only asked for the keys that get that far)
                        if (!(tk >= t_prev && tk < kt[7])) return;
                        if (tk == t_prev && !(k > k_prev && k_prev != 0xFFFFFFFFu)) return;
                        const float x = tk;
                        const bool c0 = x < kt[0], c1 = x < kt[1], c2 = x < kt[2], c3 = x < kt[3], c4 = x < kt[4], c5 = x < kt[5], c6 = x < kt[6], c7 = x < kt[7];
                        ki[7] = c6 ? ki[6] : (c7 ? k : ki[7]), kt[7] = __builtin_amdgcn_fmed3f(x, kt[6], kt[7]);
                        ki[6] = c5 ? ki[5] : (c6 ? k : ki[6]), kt[6] = __builtin_amdgcn_fmed3f(x, kt[5], kt[6]);
                        ki[5] = c4 ? ki[4] : (c5 ? k : ki[5]), kt[5] = __builtin_amdgcn_fmed3f(x, kt[4], kt[5]);
                        ki[4] = c3 ? ki[3] : (c4 ? k : ki[4]), kt[4] = __builtin_amdgcn_fmed3f(x, kt[3], kt[4]);
                        ki[3] = c2 ? ki[2] : (c3 ? k : ki[3]), kt[3] = __builtin_amdgcn_fmed3f(x, kt[2], kt[3]);
                        ki[2] = c1 ? ki[1] : (c2 ? k : ki[2]), kt[2] = __builtin_amdgcn_fmed3f(x, kt[1], kt[2]);
                        ki[1] = c0 ? ki[0] : (c1 ? k : ki[1]), kt[1] = __builtin_amdgcn_fmed3f(x, kt[0], kt[1]);
                        ki[0] = c0 ? k : ki[0], kt[0] = fminf(x, kt[0]);
                    };
                    // two 16-B loads per 8 keys (cand_cap is a multiple of 8, so runs are 32-B aligned), in flight together
                    const uint32_t nbase = min(cnt, v.cand_cap);
                    uint32_t k = 0;
                    for (; k + 16 <= nbase; k += 16) { // sixteen keys per round trip (four 16-B loads in flight)
                        const float4 ka = EGR_KEY_Q(lane, k), kb = EGR_KEY_Q(lane, k + 4);
                        const float4 kc = EGR_KEY_Q(lane, k + 8), kd = EGR_KEY_Q(lane, k + 12);
                        consider(ka.x, k), consider(ka.y, k + 1), consider(ka.z, k + 2), consider(ka.w, k + 3);
                        consider(kb.x, k + 4), consider(kb.y, k + 5), consider(kb.z, k + 6), consider(kb.w, k + 7);
                        consider(kc.x, k + 8), consider(kc.y, k + 9), consider(kc.z, k + 10), consider(kc.w, k + 11);
                        consider(kd.x, k + 12), consider(kd.y, k + 13), consider(kd.z, k + 14), consider(kd.w, k + 15);
                    }
                    if (k + 8 <= nbase) {
                        const float4 ka = EGR_KEY_Q(lane, k), kb = EGR_KEY_Q(lane, k + 4);
                        consider(ka.x, k), consider(ka.y, k + 1), consider(ka.z, k + 2), consider(ka.w, k + 3);
                        consider(kb.x, k + 4), consider(kb.y, k + 5), consider(kb.z, k + 6), consider(kb.w, k + 7);
                        k += 8;
                    }
                    if (k < nbase) { // the last, partial chunk in ONE round trip too (the run is padded to a multiple of 8: the loads stay inside it;
                                     // a key-by-key tail costs up to seven dependent fetches per scan - as many as the rest of a 29-entry list)
                        const float4 ka = EGR_KEY_Q(lane, k), kb = EGR_KEY_Q(lane, k + 4);
                        const uint32_t left = nbase - k; // 1..7
                        const float inf = 3.4028235e38f; // (never smaller than the 8th key kept: not inserted)
                        consider(ka.x, k), consider(left > 1u ? ka.y : inf, k + 1), consider(left > 2u ? ka.z : inf, k + 2), consider(left > 3u ? ka.w : inf, k + 3);
                        consider(left > 4u ? kb.x : inf, k + 4), consider(left > 5u ? kb.y : inf, k + 5), consider(left > 6u ? kb.z : inf, k + 6);
                        k = nbase;
                    }
                    for (; k < cnt; k++) consider(v.ext_keys[(size_t)ext * EGR_EXT_BLOCK + (k - v.cand_cap)], k); // the extension block (rare)
                    if (ki[0] == 0xFFFFFFFFu || !(kt[0] < far_plane)) running = false; // :81, :91-93
                }
                EGR_STATS(const unsigned long long tcs1 = __builtin_amdgcn_s_memtime(); tc_scan += tcs1 - tcs0;)
                if (__ballot(running) == 0ull) break;
                if (GRADS && recording) { // one arena block per batch per wave
                    // (blocks are taken from the arena's bump counter EGR_ARENA_CHUNK at a time and handed out from the wave's own run: every batch used to wait
                    // for a returning atomic on ONE word that ~ 110 k batches per launch go through - the same atomic unit, 12 ns apiece)
                    if (arena_next == arena_end) {
                        uint32_t b0 = 0;
                        if (lane == 0) b0 = atomicAdd(v.control + CW_HIT_BUMP, (uint32_t)EGR_ARENA_CHUNK);
                        arena_next = (uint32_t)__builtin_amdgcn_readfirstlane((int)b0), arena_end = arena_next + (uint32_t)EGR_ARENA_CHUNK;
                    }
                    const uint32_t blk = arena_next++;
                    if (blk >= v.hit_blocks_cap) {
                        recording = false;
                        if (lane == 0) atomicOr(v.control + CW_STATUS, EGR_STATUS_HIT_ARENA_OVERFLOW);
                    } else {
                        if (lane == 0) v.hit_arena[(size_t)blk * (EGR_HIT_BLOCK_ROWS + 1) * EGR_WAVE] = make_float4(u2f(last_block), 0, 0, 0);
                        last_block = cur_block = blk;
                    }
                }
                // the batch's eight (alpha, record) pairs are fetched together (a fetch for a hit the ray never reaches - it may stop at
                // the transmittance threshold - reads valid memory and is dropped): one dependent round trip instead of eight
                EGR_STATS(const unsigned long long tcs2 = __builtin_amdgcn_s_memtime(); tc_alloc += tcs2 - tcs1;)
                float2 av_[8];
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    av_[j] = make_float2(0.0f, 0.0f);
                    if (running && ki[j] != 0xFFFFFFFFu) av_[j] = ki[j] < v.cand_cap ? vals[EGR_VAL_AT(lane, ki[j])] : v.ext_vals[(size_t)ext * EGR_EXT_BLOCK + (ki[j] - v.cand_cap)];
                }
                // The batch in two passes. (1) registers only: which hits are composited, their weights, the transmittance chain, the arena
                // rows - everything that runs along the ray and needs nothing but the alphas. (2) the appearance of the composited hits,
                // FOUR AT A TIME: their 40-B records are independent fetches once pass 1 has said which hits count (one dependent round trip
                // per four hits instead of one per hit - a 22-hit ray of the dense-init cloud paid 22 of them), accumulated in hit order.
#if defined(__HIP_DEVICE_COMPILE__)
                // ALL eight fetches land here, in front of pass 1. Stores count in vmcnt on this ISA and the counter retires in order: left to the compiler, the
                // wait for av_[j + 1] sits behind hit j's (conditional) arena store, is a wait for everything - and every hit of a batch waited for the
                // previous hit's store to be acknowledged (pass 1: 2.6 G of the dense-init launch's 30 G wave-cycles for ~ 160 instructions per batch).
                asm volatile("" ::"v"(av_[0].x), "v"(av_[0].y), "v"(av_[1].x), "v"(av_[1].y), "v"(av_[2].x), "v"(av_[2].y), "v"(av_[3].x), "v"(av_[3].y));
                asm volatile("" ::"v"(av_[4].x), "v"(av_[4].y), "v"(av_[5].x), "v"(av_[5].y), "v"(av_[6].x), "v"(av_[6].y), "v"(av_[7].x), "v"(av_[7].y));
#endif
                EGR_STATS(const unsigned long long tcs3 = __builtin_amdgcn_s_memtime(); tc_av += tcs3 - tcs2;)
                float wj[8];
                uint32_t pj[8], runm = 0u;
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    wj[j] = 0.0f, pj[j] = 0u;
                    if (running && (ki[j] == 0xFFFFFFFFu || !(kt[j] < far_plane))) running = false; // list exhausted / beyond zfar
                    if (running) {
                        const float best = kt[j];
                        t_prev = best;
                        k_prev = ki[j];
                        const float2 av = av_[j];
                        float alpha = av.x;
                        uint32_t pos = f2u(av.y); // record index (sorted position)
                        float next_T = T * (1.0f - alpha);       // :108
                        float weight = T - next_T;               // :109
                        wj[j] = weight, pj[j] = pos, runm |= 1u << j;
                        c_depth += best * weight;
                        T = next_T;
                        nhits++;
                        if (GRADS && recording)
                            v.hit_arena[((size_t)cur_block * (EGR_HIT_BLOCK_ROWS + 1) + 1 + j) * EGR_WAVE + lane] = make_float4(u2f(pos), best, alpha, T);
                        if (T < transmittance_threshold || nhits >= EGR_MAX_COMPOSITED_PER_RAY) running = false; // :131-134, :55
                    }
                }
                EGR_STATS(const unsigned long long tcs4 = __builtin_amdgcn_s_memtime(); tc_p1 += tcs4 - tcs3;)
                if constexpr (OBJ) {
                    // (k_forward_objects) instead of the appearance: the membership words of four hits at a time - record order, one independent load each - and
                    // every hit's weight added, in hit order, to the sum of each object its row belongs to. The sums live in LDS and are addressed by the
                    // lowest remaining bit (a row is in one or two objects): no array in registers, nothing indexed in private memory.
#pragma unroll
                    for (int g4 = 0; g4 < 8; g4 += 4) {
                        uint32_t M[4];
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            M[j] = 0u;
                            if ((runm >> (g4 + j)) & 1u) M[j] = oq.pos_bits[pj[g4 + j]];
                        }
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            const float weight = wj[g4 + j];
                            for (uint32_t m = M[j]; m != 0u; m &= m - 1u) oacc[(uint32_t)__builtin_ctz(m) * EGR_WAVE + (uint32_t)lane] += weight;
                        }
                    }
                } else {
#pragma unroll
                for (int g4 = 0; g4 < 8; g4 += 4) {
                    float4 A0[4], A1[4];
                    float2 A2[4];
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        A0[j] = make_float4(0, 0, 0, 0), A1[j] = A0[j], A2[j] = make_float2(0, 0);
                        if ((runm >> (g4 + j)) & 1u) {
                            const uint32_t pos = pj[g4 + j];
                            A0[j] = app[2 * pos], A1[j] = app[2 * pos + 1];
                            A2[j] = *reinterpret_cast<const float2 *>(v.inst_w + 4 * pos + 3); // (f0.z, roughness) of the live quarter
                        }
                    }
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        if ((runm >> (g4 + j)) & 1u) {
                            const float weight = wj[g4 + j];
                            const float4 a0 = A0[j], a1 = A1[j];
                            c_rgb = c_rgb + mk3(a0.x, a0.y, a0.z) * weight;
                            c_n = c_n + mk3(a0.w, a1.x, a1.y) * weight;
                            c_f0 = c_f0 + mk3(a1.z, a1.w, A2[j].x) * weight;
                            c_rough += A2[j].y * weight;
                        }
                    }
                }
                }
                EGR_STATS(asm volatile("" ::"v"(c_rough)); tc_app += __builtin_amdgcn_s_memtime() - tcs4;)
            }
            EGR_STATS(if (lane == 0 && step == 0) {
                unsigned long long *d = diag64(v.control, DG_COMP_SCAN_CYC);
                atomicAdd(d, tc_scan), atomicAdd(d + 1, tc_alloc), atomicAdd(d + 2, tc_av), atomicAdd(d + 3, tc_p1), atomicAdd(d + 4, tc_app);
            })
            if (GRADS) {
                // arena exhausted: forward results stay exact, the backward skips THIS STEP of this task, all of it (no chain head, no hits; the status flag is
                // raised): the gradients of an overflowing launch are those of its recorded (task, step)s (tests/test_hip_overflow.py). Either store alone makes
                // the backward skip; the hit count is also what egr_debug_get_step_hits reports.
                if (lane == 0) v.task_last_block[chain_head] = recording ? last_block : 0xFFFFFFFFu;
                if (tg.inside) S.st(SF(step, S_NHITS), u2f(recording ? nhits : 0u));
            }
        }
        if (overflow && active) atomicOr(v.control + CW_STATUS, EGR_STATUS_CANDIDATE_OVERFLOW);

        EGR_STATS(if (lane == 0) atomicAdd(diag64(v.control, DG_TRAVERSAL_CYC, step > 0), tm1 - tm0), atomicAdd(diag64(v.control, DG_COMPOSITE_CYC, step > 0), __builtin_amdgcn_s_memtime() - tm1);)
        // ---- raw step results; R4/R5 (tail renormalisation, bounce sampling) follow in step_epilogue_lane (egr_epilogue.hpp),
        // which is compiled without fma contraction (see the note there).
        if constexpr (OBJ) {
            // (k_forward_objects) the tile's end: no ray state, no statistics, no step epilogue. Each pixel of the tile turns its sums into the R4 values of the
            // primary step (egr_epilogue.hpp: mask_tail / mask_value, unfused) and writes masks[j][pixel] for every requested object, then the
            // non-zero set and the largest coverage from the same registers (strict '>': ties go to the lowest index, a NaN never wins).
            if (tg.inside) {
                const MaskTail mt = mask_tail(T, full_T, *v.cfg.eps_forward_normalization);
                uint32_t hit = 0u;
                int32_t top = -1;
                float best = -__builtin_inff();
                for (uint32_t j = 0; j < oq.num_bits; j++) {
                    const float m = mask_value(oacc[j * EGR_WAVE + (uint32_t)lane], mt);
                    oq.masks[(size_t)j * v.num_pixels + tg.pixel_id] = m;
                    if (m != 0.0f) hit |= 1u << j;
                    if (m > best) best = m, top = (int32_t)j;
                }
                if (oq.hit) oq.hit[tg.pixel_id] = hit;
                if (oq.top) oq.top[tg.pixel_id] = hit != 0u ? top : -1;
            }
        }
        if (!OBJ && active) {
            S.st3(SF(step, S_RGB), c_rgb), S.st(SF(step, S_DEPTH), c_depth), S.st3(SF(step, S_NORMAL), c_n);
            S.st3(SF(step, S_F0), c_f0), S.st(SF(step, S_ROUGH), c_rough), S.st(SF(step, S_T), T), S.st(SF(step, S_TTOT), full_T);
            if (step == 0) {
                S.st3(F_RAY_O, ro), S.st3(F_RAY_D, rd);
                S.st(F_SEED, u2f(seed));
            }
            if (last_frame) { // (a batch: its last frame only)
                v.stats.num_accumulated_per_pixel[tg.pixel_id] = (int32_t)nhits;  // forward_pass.cu:140 (last step wins)
                if (step == 0) v.stats.num_traversed_per_pixel[tg.pixel_id] = (int32_t)traversed;
                else v.stats.num_traversed_per_pixel[tg.pixel_id] += (int32_t)traversed; // forward_pass.cu:46
            }
        }
        EGR_TIMES(if (step == EGR_TASK_TIMES && tg.inside) { // the tile's first pixel carries the task's start / end time of one step (which must be the last), 10 ns ticks; the second the walk / selection boundary;
            // pixels 2 .. 4: the owner's walk batches / evaluation batches, offers made / batches that left a tall stack, ticks waited for helpers / longest candidate list
            if (lane == 0) v.stats.num_traversed_per_pixel[tg.pixel_id] = EGR_STAMP31(tt0), v.stats.num_accumulated_per_pixel[tg.pixel_id] = EGR_STAMP31(__builtin_amdgcn_s_memrealtime());
            if (lane == 1) v.stats.num_traversed_per_pixel[tg.pixel_id] = EGR_STAMP31(tt_mid);
            const uint32_t cmax = wave_max_u32(active ? cnt : 0u);
            tt_batches = (uint32_t)__shfl((int)tt_batches, 0), tt_evals = (uint32_t)__shfl((int)tt_evals, 0), tt_offers = (uint32_t)__shfl((int)tt_offers, 0), tt_tall = (uint32_t)__shfl((int)tt_tall, 0);
            if (lane == 2) v.stats.num_traversed_per_pixel[tg.pixel_id] = (int32_t)tt_batches, v.stats.num_accumulated_per_pixel[tg.pixel_id] = (int32_t)tt_evals;
            if (lane == 3) v.stats.num_traversed_per_pixel[tg.pixel_id] = (int32_t)tt_offers, v.stats.num_accumulated_per_pixel[tg.pixel_id] = (int32_t)tt_tall;
            if (lane == 4) v.stats.num_traversed_per_pixel[tg.pixel_id] = (int32_t)tt_wait, v.stats.num_accumulated_per_pixel[tg.pixel_id] = (int32_t)cmax;
        })
