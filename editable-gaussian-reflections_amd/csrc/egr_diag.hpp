// The diagnostics layer of the trace kernels: the build-time switches, the statement macros the kernels carry them in, the control words they count in and
// the host table that prints those. A build with any switch is a VARIANT (build.py: build/variants/<name>/), never the product; in the product build every
// macro below expands to nothing and the kernels' code is what it is without this header.
//
//   EGR_TRAVERSAL_STATS        walk / evaluation counters and s_memtime sums per phase of both chains, summed over the launch in the DiagSlot words;
//                              egr_get_counters prints them under EGR_PRINT_TRAVERSAL_STATS=1 (tools/stats_ab.sh)
//   EGR_TASK_TIMES=<step>      s_memrealtime stamps (10 ns ticks, modulo 2^31) of ONE forward step of every task, smuggled out in the statistics images of
//                              the tile's first pixels (tools/task_times.py: the step must be the launch's last); = 9: of the whole forward chain - start,
//                              end of every step, leaves of the primary step (tools/chain_times.py); = 8: of the backward chain (tools/bwd_times.py)
//   EGR_DEBUG_PIXEL=<id>       printf of the candidate list of one pixel's primary ray (forward_task.inc)
//   EGR_DEBUG_LIST             printf of every ray whose list's transmittance product disagrees with its full_T (forward_task.inc)
#pragma once
#include <stdio.h>

#include "egr_internal.hpp"
#ifdef EGR_TRAVERSAL_STATS
#define EGR_STATS(...) __VA_ARGS__
#else
#define EGR_STATS(...)
#endif
#ifdef EGR_TASK_TIMES
#define EGR_TIMES(...) __VA_ARGS__
#else
#define EGR_TIMES(...)
#endif
#define EGR_TIMES_IS(n, ...) EGR_TIMES(if (EGR_TASK_TIMES == (n)) { __VA_ARGS__ }) // statements of the = 8 / = 9 builds (what they declare: EGR_TIMES)
#if defined(EGR_TRAVERSAL_STATS) || defined(EGR_TASK_TIMES) // the pair walk's WalkStats (trace.hip) feed both
#define EGR_WALK_STATS 1
#define EGR_WALK(...) __VA_ARGS__
#else
#define EGR_WALK(...)
#endif
#define EGR_STAMP31(t) ((int32_t)((t) & 0x7FFFFFFFull)) // a 64-bit time as a statistics image holds it

// The diagnostic control words [DG_BEGIN, DG_END) of ControlWord (egr_internal.hpp); EGR_DIAG_TABLE below says what each holds. k_prologue zeroes the whole range in
// every launch of EVERY build and seeds DG_STEP_EXIT; everything else is written by EGR_TRAVERSAL_STATS builds only.
enum DiagSlot : int {
    DG_BEGIN = 32, // per step class, 64-bit: primary at the slot, bounce DG_CLASS_STRIDE words on (56 .. 79); the backward's five words are added through one pointer (backward_chain.hpp: primary_hits)
    DG_VISITS = 32, DG_LEAF_HITS = 34, DG_WALK_ITERS = 36, DG_EVAL_ROUNDS = 38, DG_TRAVERSAL_CYC = 40, DG_COMPOSITE_CYC = 42, DG_LEAF_EVAL_CYC = 44, DG_BWD_MATH_CYC = 46 /* x 5 */, DG_CLASS_STRIDE = 24,
    DG_EPILOGUE_CYC = 80, DG_CHAIN_CYC = 82, DG_FILTER_CYC = 84, DG_FILTER_LEAVES = 86, DG_COMP_SCAN_CYC = 88 /* x 5, one pointer again (forward_task.inc) */, // once per launch, 64-bit
    DG_LIST_HIST = 98 /* x 7 */, DG_BWD_ROW_GROUPS = 106 /* x 3, 64-bit, one pointer (backward_chain.hpp: primary_hits) */, DG_TEAM_OFFERS = 124, DG_TEAM_HELPED = 125, DG_TEAM_HELP_ITERS = 126, DG_TEAM_TALL = 127, // once per launch, 32-bit
    DG_STEP_EXIT = 112, // 32-bit x 12: min / max seeds of a per-step wave exit time that no kernel records any more; the prologue still writes them
    DG_END = 128
};
static_assert((int)DG_BEGIN > (int)CW_LIFE_LAUNCHES && (int)DG_END <= (int)CW_HIT_BUMP, "the diagnostic words lie between the counters and the bump allocators");
static_assert(CW_HIT_BUMP % 32 == 0 && CW_EXT_BUMP % 32 == 0 && CW_EXT_BUMP >= CW_HIT_BUMP + 32 && CW_COUNT >= CW_EXT_BUMP + 32, "DESIGN.md: a word many waves update with atomics starts a 128-B line that holds nothing else");
// ---- host: what egr_get_counters prints under EGR_PRINT_TRAVERSAL_STATS ---------------------------------------------------------------------------------
// One line per run of entries of one group: [egr stats <group>] <label> <value>, ... bits: 32 / 64; per_class ("x 2"): a line for "primary", one for "bounce".
enum DiagKind : uint8_t { DK_COUNT, DK_CYCLES /* s_memtime, summed over waves */ };
struct DiagEntry { int slot, bits; DiagKind kind; bool per_class; const char *group, *label; };
constexpr DiagEntry EGR_DIAG_TABLE[] = {
    {DG_VISITS, 64, DK_COUNT, true, "", "lane node visits"},
    {DG_LEAF_HITS, 64, DK_COUNT, true, "", "lane leaf-box hits"},
    {DG_WALK_ITERS, 64, DK_COUNT, true, "", "wave inner iterations"},
    {DG_EVAL_ROUNDS, 64, DK_COUNT, true, "", "wave outer rounds"},
    {DG_TRAVERSAL_CYC, 64, DK_CYCLES, true, "", "traversal"},
    {DG_COMPOSITE_CYC, 64, DK_CYCLES, true, "", "composite"},
    {DG_LEAF_EVAL_CYC, 64, DK_CYCLES, true, "", "of the traversal: leaf evaluation (frustum walk)"},
    {DG_BWD_MATH_CYC, 64, DK_CYCLES, true, "backward ", "per-hit math"},
    {DG_BWD_MATH_CYC + 2, 64, DK_CYCLES, true, "backward ", "neighbour combine + LDS table"},
    {DG_BWD_MATH_CYC + 4, 64, DK_CYCLES, true, "backward ", "wide adds"},
    {DG_BWD_MATH_CYC + 6, 64, DK_CYCLES, true, "backward ", "table flush"},
    {DG_BWD_MATH_CYC + 8, 64, DK_COUNT, true, "backward ", "hit rows"},
    {DG_EPILOGUE_CYC, 64, DK_CYCLES, false, "forward chain", "step epilogues"},
    {DG_CHAIN_CYC, 64, DK_CYCLES, false, "forward chain", "whole chains (task pull to end)"},
    {DG_FILTER_CYC, 64, DK_CYCLES, false, "primary leaf filter", "sphere / pyramid test"},
    {DG_FILTER_LEAVES, 64, DK_COUNT, false, "primary leaf filter", "leaves before the test"},
    {DG_COMP_SCAN_CYC, 64, DK_CYCLES, false, "primary composite", "selection scans"},
    {DG_COMP_SCAN_CYC + 2, 64, DK_CYCLES, false, "primary composite", "arena block"},
    {DG_COMP_SCAN_CYC + 4, 64, DK_CYCLES, false, "primary composite", "alpha / record fetch"},
    {DG_COMP_SCAN_CYC + 6, 64, DK_CYCLES, false, "primary composite", "pass 1"},
    {DG_COMP_SCAN_CYC + 8, 64, DK_CYCLES, false, "primary composite", "appearance pass"},
    {DG_LIST_HIST, 32, DK_COUNT, false, "primary lists", "tiles by their longest candidate list: <=16"},
    {DG_LIST_HIST + 1, 32, DK_COUNT, false, "primary lists", "<=24"},
    {DG_LIST_HIST + 2, 32, DK_COUNT, false, "primary lists", "<=32"},
    {DG_LIST_HIST + 3, 32, DK_COUNT, false, "primary lists", "<=40"},
    {DG_LIST_HIST + 4, 32, DK_COUNT, false, "primary lists", "<=48"},
    {DG_LIST_HIST + 5, 32, DK_COUNT, false, "primary lists", "<=64"},
    {DG_LIST_HIST + 6, 32, DK_COUNT, false, "primary lists", "longer"},
    {DG_BWD_ROW_GROUPS, 64, DK_COUNT, false, "backward primary", "lanes with a hit"},
    {DG_BWD_ROW_GROUPS + 2, 64, DK_COUNT, false, "backward primary", "pointer-jumping steps"},
    {DG_BWD_ROW_GROUPS + 4, 64, DK_COUNT, false, "backward primary", "leaders"},
    {DG_TEAM_OFFERS, 32, DK_COUNT, false, "team", "offers made"},
    {DG_TEAM_HELPED, 32, DK_COUNT, false, "team", "offers walked by helpers"},
    {DG_TEAM_HELP_ITERS, 32, DK_COUNT, false, "team", "their walk iterations"},
    {DG_TEAM_TALL, 32, DK_COUNT, false, "team", "owner walk iterations that left >= EGR_DONATE_MIN pairs on the stack"},
};
constexpr bool egr_diag_layout_ok() { // the table in ascending order (so: disjoint), per-class entries inside the first class's block, the others behind both blocks and clear of the seeded words
    int end = DG_BEGIN;
    for (const DiagEntry &d : EGR_DIAG_TABLE) {
        const int lo = d.per_class ? DG_BEGIN : DG_BEGIN + 2 * DG_CLASS_STRIDE, hi = d.per_class ? DG_BEGIN + DG_CLASS_STRIDE : DG_END, e = d.slot + d.bits / 32;
        if (d.slot < end || d.slot < lo || e > hi || (d.bits == 64 && d.slot % 2 != 0) || (e > DG_STEP_EXIT && d.slot < DG_STEP_EXIT + 12)) return false;
        end = e;
    }
    return true;
}
static_assert(egr_diag_layout_ok(), "diagnostic slots: inside [DG_BEGIN, DG_END), disjoint, 64-bit ones 8-byte aligned");

inline void egr_diag_print(const uint32_t *w) { // w: the control block as the host read it
    const int n = (int)(sizeof(EGR_DIAG_TABLE) / sizeof(EGR_DIAG_TABLE[0]));
    for (int i = 0, j; i < n; i = j) {
        const DiagEntry &g = EGR_DIAG_TABLE[i];
        for (j = i + 1; j < n && __builtin_strcmp(EGR_DIAG_TABLE[j].group, g.group) == 0; j++) {}
        for (int k = 0; k <= (g.per_class ? 1 : 0); k++) {
            fprintf(stderr, "[egr stats %s%s]", g.group, !g.per_class ? "" : k ? "bounce" : "primary");
            for (int e = i; e < j; e++) {
                const int s = EGR_DIAG_TABLE[e].slot + k * DG_CLASS_STRIDE;
                const unsigned long long x = EGR_DIAG_TABLE[e].bits == 64 ? (unsigned long long)w[s] | ((unsigned long long)w[s + 1] << 32) : w[s];
                fprintf(stderr, "%s %s %llu%s", e > i ? "," : "", EGR_DIAG_TABLE[e].label, x, EGR_DIAG_TABLE[e].kind == DK_CYCLES ? " wave-cycles" : "");
            }
            fputc('\n', stderr);
        }
    }
}

#if defined(EGR_TRAVERSAL_STATS) && defined(__HIPCC__)
__device__ __forceinline__ unsigned long long *diag64(uint32_t *control, int slot, bool bounce = false) { return reinterpret_cast<unsigned long long *>(control + slot + (bounce ? DG_CLASS_STRIDE : 0)); }
#endif
