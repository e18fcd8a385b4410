// g2g_plan.h -- the host-side decisions of a batch as plain values.  Of a run: which variant slot is which kernel, how the CUs are
// shared out, the list of persistent launches, the text of a time-out report, and the LDS plan of the v6 launches.  Of prepare: the
// shape of the batch (tile widths, strip heights, v6 or not), the kernel of each DP, and its queues (tiles, flag image, LDS plans).
// Plain C++17 without HIP types (it compiles with g++: tests/host/plan_main.cc and v6_layout_main.cc pin all of it without a GPU);
// g2g_engine.hip fills the facts and executes what is planned here.
#ifndef G2G_PLAN_H
#define G2G_PLAN_H
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <string>
#include <utility>
#include <vector>
#include "g2g_lds.h"                 // V6Lds, the v6 window constants, v3_pitch, v6_inline_dw (shared with the kernels)

#define G2G_NVAR 32                 // variant slots
#define G2G_PLAN_HDR 24             // G2G_HDR of g2g_strip.h (the engine asserts that they agree)
#define G2G_NVS 8                   // launch streams of a context (HIP multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues, 4 by default: bench.py asks for 8)
static const size_t V2_LDS_MAX = 160 * 1024;

// ---- (a) the variant table -----------------------------------------------------------------------------------------
// A variant slot is one queue and one persistent launch.  The queue heads of slots [0, G2G_HDR) are the first G2G_HDR words
// of d_flags (g2g_strip.h), those of the bonus-aware instantiations (_ib, [G2G_HDR, G2G_NVAR)) live at d_flags + xq_off.
// The family's number is the kernel generation of DevProb::v2_ok and of g2g_batch_paths' tally.
enum G2GFamily { G2G_NONE = 0, G2G_V2 = 1, G2G_V3_LDS = 2, G2G_V3R = 3, G2G_V6 = 6, G2G_V7 = 7, G2G_V8 = 8 };
enum G2GRecord { G2G_REC_NONE = 0, G2G_REC_HF = 1, G2G_REC_PF = 2 };
struct G2GVariant {
    const char *name;               // the kernel
    G2GFamily fam;
    G2GRecord rec;
    bool noll3, ib;
    int cls;                        // v6: footprint class A / B / C = 0 / 1 / 2 (the kernel is the same, the LDS plan is the launch's)
    double cost;                    // relative cost of a cell on this kernel for Noll 2 (what the CU shares are proportional to)
};
static const G2GVariant G2G_VARIANT[G2G_NVAR] = {
    {"g2g_v2_hf2", G2G_V2, G2G_REC_HF, false, false, -1, 2.0},        {"g2g_v2_hf3", G2G_V2, G2G_REC_HF, true, false, -1, 2.0},
    {"g2g_v2_pf2", G2G_V2, G2G_REC_PF, false, false, -1, 5.0},        {"g2g_v2_pf3", G2G_V2, G2G_REC_PF, true, false, -1, 5.0},
    {"g2g_v3_hf2", G2G_V3_LDS, G2G_REC_HF, false, false, -1, 2.5},    {"g2g_v3_hf3", G2G_V3_LDS, G2G_REC_HF, true, false, -1, 2.5},
    {"", G2G_NONE, G2G_REC_NONE, false, false, -1, 0},                {"", G2G_NONE, G2G_REC_NONE, false, false, -1, 0},       // (_pf strips with one lane per cell: v6)
    {"g2g_v3r_hf2", G2G_V3R, G2G_REC_HF, false, false, -1, 1.0},      {"g2g_v3r_hf3", G2G_V3R, G2G_REC_HF, true, false, -1, 1.0},
    {"", G2G_NONE, G2G_REC_NONE, false, false, -1, 0},                {"", G2G_NONE, G2G_REC_NONE, false, false, -1, 0},
    {"g2g_v6_pf2", G2G_V6, G2G_REC_PF, false, false, 0, 2.7},         {"g2g_v6_pf3", G2G_V6, G2G_REC_PF, true, false, 0, 2.7},
    {"g2g_v6_pf2", G2G_V6, G2G_REC_PF, false, false, 1, 2.7},         {"g2g_v6_pf3", G2G_V6, G2G_REC_PF, true, false, 1, 2.7},
    {"g2g_v7_ngp2", G2G_V7, G2G_REC_NONE, false, false, -1, 0.8},     {"g2g_v7_ngp3", G2G_V7, G2G_REC_NONE, true, false, -1, 0.8},
    {"g2g_v8_ntv2", G2G_V8, G2G_REC_NONE, false, false, -1, 1.2},     {"g2g_v8_ntv3", G2G_V8, G2G_REC_NONE, true, false, -1, 1.2},
    {"g2g_v6_pf2", G2G_V6, G2G_REC_PF, false, false, 2, 2.7},         {"g2g_v6_pf3", G2G_V6, G2G_REC_PF, true, false, 2, 2.7},
    {"", G2G_NONE, G2G_REC_NONE, false, false, -1, 0},                {"", G2G_NONE, G2G_REC_NONE, false, false, -1, 0},
    {"g2g_v7_ngp2_ib", G2G_V7, G2G_REC_NONE, false, true, -1, 0.8},   {"g2g_v7_ngp3_ib", G2G_V7, G2G_REC_NONE, true, true, -1, 0.8},
    {"g2g_v2_hf2_ib", G2G_V2, G2G_REC_HF, false, true, -1, 2.0},      {"g2g_v2_hf3_ib", G2G_V2, G2G_REC_HF, true, true, -1, 2.0},
    {"g2g_v2_pf2_ib", G2G_V2, G2G_REC_PF, false, true, -1, 5.0},      {"g2g_v2_pf3_ib", G2G_V2, G2G_REC_PF, true, true, -1, 5.0},
    {"g2g_v8_ntv2_ib", G2G_V8, G2G_REC_NONE, false, true, -1, 1.2},   {"g2g_v8_ntv3_ib", G2G_V8, G2G_REC_NONE, true, true, -1, 1.2},
};
// The order in which a run launches its non-empty slots: v2 and its _ib; v3 / v3r (the _hf launch goes before the _pf launches of
// v6 on purpose: submitted behind them -- whose persistent workgroups hold the LDS of every CU until their queues are empty -- it
// runs after them instead of beside them: 845 ms per bench sweep instead of 757); v6, the larger footprint first; v7, v8, their _ib.
static const int G2G_LAUNCH_ORDER[] = {0, 1, 2, 3, 26, 27, 28, 29, 4, 5, 6, 7, 8, 9, 10, 11, 21, 20, 15, 14, 13, 12, 16, 17, 18, 19, 24, 25, 30, 31};
static const int G2G_NLAUNCH_ORDER = (int) (sizeof G2G_LAUNCH_ORDER / sizeof G2G_LAUNCH_ORDER[0]);

static inline double variant_cost(int slot) { return G2G_VARIANT[slot].cost * (G2G_VARIANT[slot].noll3 ? 1.4 : 1.0); }
static inline bool variant_is_v3(int slot) { return G2G_VARIANT[slot].fam == G2G_V3_LDS || G2G_VARIANT[slot].fam == G2G_V3R; }
// index of a slot within its family's per-batch arrays: v3 / v3r -> v3lds[8] and the builder's need[8] (also the number the v3
// debug lines and ONLY_VAR speak of), v6 -> v6lds[6] / twin[6] (footprint class x 2 + Noll 3); -1 for the other families
static inline int variant_v3_index(int slot) { return variant_is_v3(slot) ? (G2G_VARIANT[slot].fam == G2G_V3R ? 4 : 0) + (G2G_VARIANT[slot].noll3 ? 1 : 0) : -1; }
static inline int variant_v6_index(int slot) { return G2G_VARIANT[slot].fam == G2G_V6 ? 2 * G2G_VARIANT[slot].cls + (G2G_VARIANT[slot].noll3 ? 1 : 0) : -1; }
// The slot of a DP: its kernel generation (DevProb::v2_ok), DP kind (2: _pf records, else _hf where the family has both), Noll,
// whether it carries a bonus table, and for v6 its footprint class; -1 where no kernel exists for the combination.
static inline int variant_slot(int generation, int kind, int noll, bool ib, int v6cls)
{
    for (int s = 0; s < G2G_NVAR; ++s) {
        const G2GVariant &r = G2G_VARIANT[s];
        if (r.fam == G2G_NONE || (int) r.fam != generation || r.noll3 != (noll == 3) || r.ib != ib) continue;
        if (r.fam == G2G_V6 ? r.cls != v6cls : (r.rec != G2G_REC_NONE && r.rec != (kind == 2 ? G2G_REC_PF : G2G_REC_HF))) continue;
        return s;
    }
    return -1;
}
// g2g_batch_paths' number of a generation: 1 g2g_forward_kernel, 2 the 8-lanes-per-cell strips, 3 v3 / v3r, 6, 7, 8
static inline int family_path(int generation) { return generation == G2G_NONE ? 1 : generation == G2G_V2 ? 2 : generation == G2G_V3_LDS || generation == G2G_V3R ? 3 : generation; }

// ---- what a run knows about its batch ------------------------------------------------------------------------------
struct LdsFacts { int total, svals, rows, black; };           // of a V3Lds / V6Lds plan
struct RunFacts {
    int cnt[G2G_NVAR];              // queue entries per slot
    long long cells[G2G_NVAR];      // in-band cells per slot
    int ncu;
    size_t lds2, lds2p;
    int v2_threads, v2_sweep, v3_sweep, v2_cols, v3_cols;
    LdsFacts v3[8], v6[6];
    int v2_wpc, v3_wpc, v6_wpc;     // options V2_WPC / V3_WPC / V6_WPC when in 1 .. 32, else 0
    bool only_var_set; int only_var;                          // option ONLY_VAR (profiling aid)
    bool no_simblk, no_prostage, parallel_hf;
    size_t pro_lds_bytes;           // PRO_LDS_BYTES of g2g_kernels_v2.hip
    size_t simblk_bytes;            // column-score scratch of one workgroup (G2G_SIMBLK_STRIDE doubles)
};
static inline int plan_pro_off(const RunFacts &f) { return f.no_prostage ? 0 : (int) ((f.lds2p + 15) & ~(size_t) 15); }
static inline int clamp_wpc(size_t lds_total, int most) { return lds_total > 0 ? std::max(1, std::min(most, (int) (V2_LDS_MAX / lds_total))) : 1; }
// resident workgroups per CU of a slot, as the CU shares see them (the *_WPC options size grids only)
static inline int share_wpc(const RunFacts &f, int slot)
{
    switch (G2G_VARIANT[slot].fam) {
    case G2G_V2: return std::max(1, std::min(2048 / f.v2_threads, (int) (V2_LDS_MAX / (f.lds2 + 4 * (size_t) f.v2_threads))));
    case G2G_V3_LDS: case G2G_V3R: return clamp_wpc((size_t) f.v3[variant_v3_index(slot)].total, 16);
    case G2G_V6: return clamp_wpc((size_t) f.v6[variant_v6_index(slot)].total, 4);
    case G2G_V7: return 16;
    case G2G_V8: return 4;
    default: return 1;
    }
}

// ---- (b) CU shares -------------------------------------------------------------------------------------------------
// The chip is cut into 32 units of 8 CUs (one CU slot of every XCD); a launch gets a contiguous range of units in proportion
// to its estimated work, capped by what its strips can occupy (see cu_share_stream in g2g_engine.hip).
struct ShareIn {
    int cnt[G2G_NVAR]; long long cells[G2G_NVAR]; int wpc[G2G_NVAR];      // per slot: queue entries, in-band cells, resident workgroups per CU
    int ncu;
    bool mode_set; int mode;        // option CU_SHARES: 0 / 1 / 2: never / for runs that fill the machine twice over / always
    bool debug, no_share_gap;
    size_t mstream_cap;             // MSTREAM_MAX
    std::vector<std::pair<int, int> > alive;                  // (lo, n) of the CU-mask streams the context holds
};
struct ShareOut { bool shares; int lo[G2G_NVAR], n[G2G_NVAR]; };
static inline void cu_share_plan(const ShareIn &in, ShareOut &out)
{
    int *sh_lo = out.lo, *sh_n = out.n;
    bool &shares = out.shares;
    shares = false;
    double work[G2G_NVAR], tot = 0;
    int need[G2G_NVAR], nl = 0;
    double demand = 0;
    bool has_v6 = false;
    for (int v = 0; v < G2G_NVAR; ++v) {
        const int cnt = in.cnt[v];
        work[v] = cnt ? (double) std::max<long long>(in.cells[v], 1) * variant_cost(v) : 0;
        need[v] = cnt ? std::min(32, std::max(1, (cnt + 8 * in.wpc[v] - 1) / (8 * in.wpc[v]))) : 0;   // units its tiles can occupy
        sh_lo[v] = 0; sh_n[v] = 0;
        if (cnt) { ++nl; tot += work[v]; demand += (double) cnt / in.wpc[v]; }
        if (cnt > 0 && G2G_VARIANT[v].fam == G2G_V6) has_v6 = true;
    }
    // Default: shares when no v6 launch is in the run -- the regime of a window of g2g_refine and of a rank's share of a sharded
    // sweep (_pf on v2 beside _hf on v3r: the two kernels slow each other down on a shared CU; 1/8 of the bench sweep 179 -> 140 ms,
    // 1/4 266 -> 245 ms, a window of the 256 x 1024 refinement 107 -> 102 ms).  Not with v6 in the run: its class of the most
    // balanced divisions is bound by its DPs' critical path, needs many CUs for a short time, and a static share leaves them idle
    // afterwards (a full sweep 1563 ms instead of 760, half of one 734 instead of 437).  CU_SHARES=0 / 1 / 2: never /
    // for runs that fill the machine twice over / always.
    const bool autosh = !in.mode_set && !has_v6;
    const bool want = in.mode_set ? in.mode != 0 : autosh;
    const bool force = (in.mode_set && in.mode >= 2) || autosh;
    // only a run that fills the machine more than twice over is partitioned, and only if every launch can have a unit
    if (!(want && in.ncu == 256 && nl >= 2 && nl <= (int) in.mstream_cap && (force || demand >= 2.0 * in.ncu) && tot > 0 && !in.debug)) return;      // (256 CUs in 8 XCDs: the mask layout the shares are written for)
    int left = 32;
    double wleft = tot;
    bool done[G2G_NVAR];
    for (int v = 0; v < G2G_NVAR; ++v) done[v] = work[v] == 0;
    // launches whose tiles cannot fill their proportional share take what they can fill; the rest is re-divided
    for (int round = 0; round < G2G_NVAR; ++round) {
        bool changed = false;
        for (int v = 0; v < G2G_NVAR; ++v) {
            if (done[v]) continue;
            const double prop = wleft > 0 ? left * work[v] / wleft : 0;
            if (need[v] <= prop) { sh_n[v] = need[v]; left -= need[v]; wleft -= work[v]; done[v] = true; changed = true; }
        }
        if (!changed) break;
    }
    int open_ = 0;
    for (int v = 0; v < G2G_NVAR; ++v) if (!done[v]) ++open_;
    if (left < open_) return;
    int given = 0;
    double frac[G2G_NVAR];
    for (int v = 0; v < G2G_NVAR; ++v) {
        frac[v] = -1;
        if (done[v]) continue;
        const double prop = left * work[v] / wleft;
        sh_n[v] = std::max(1, (int) prop);
        frac[v] = prop - (int) prop;
        given += sh_n[v];
    }
    while (given < left) {                       // largest remainders first
        int best = -1;
        for (int v = 0; v < G2G_NVAR; ++v) if (frac[v] >= 0 && (best < 0 || frac[v] > frac[best])) best = v;
        if (best < 0) break;
        ++sh_n[best]; frac[best] = -0.5; ++given;
    }
    while (given > left) {                       // (the minimum of one unit each overdrew: take from the largest)
        int big = -1;
        for (int v = 0; v < G2G_NVAR; ++v) if (!done[v] && sh_n[v] > 1 && (big < 0 || sh_n[v] > sh_n[big])) big = v;
        if (big < 0) break;
        --sh_n[big]; --given;
    }
    if (given != left) return;
    // two launches (the common case: _pf on v2 beside _hf on v3r): a split within one unit of one already in use is
    // as good, and keeps the number of queues down
    if (nl == 2) {
        int v0 = -1, v1 = -1;
        for (int v = 0; v < G2G_NVAR; ++v) if (sh_n[v]) { if (v0 < 0) v0 = v; else v1 = v; }
        if (v0 >= 0 && v1 >= 0 && sh_n[v0] + sh_n[v1] == 32) {
            // (once the context holds its fill of shares, the nearest one is taken whatever the distance: creating and
            //  destroying queues while launches are resident makes the scheduler rebuild its run list, which the waiting
            //  waves see as a pause of some 10 ms)
            const int tol = in.alive.size() + 2 > in.mstream_cap ? 32 : 1;
            int best = -1;
            for (const auto &m : in.alive) {
                if (m.first != 0 || m.second < 1 || m.second > 31 || abs(m.second - sh_n[v0]) > tol) continue;
                bool partner = false;
                for (const auto &q : in.alive) if (q.first == m.second && q.second == 32 - m.second) partner = true;
                if (partner && (best < 0 || abs(m.second - sh_n[v0]) < abs(best - sh_n[v0]))) best = m.second;
            }
            if (best > 0) { sh_n[v0] = best; sh_n[v1] = 32 - best; }
        }
    }
    // ONE UNIT OF 8 CUs STAYS EMPTY BETWEEN TWO SHARES (taken from the larger one).  Every stalled pipeline head of round 4
    // (20 of 20 events) was held by one of the LAST 24 workgroups of the `_pf` launch's 600 resident
    // ones -- the three workgroups on each CU of the share's last unit, next to the other launch's share; with the gap:
    // 5 whole refinements (4360 windows) without an event against 0.6 events per run before, 0.5 % slower.
    // NO_SHARE_GAP restores adjacent shares.
    const int gap = (!in.no_share_gap && nl == 2) ? 1 : 0;
    if (gap) { int vb = -1; for (int v = 0; v < G2G_NVAR; ++v) if (sh_n[v] && (vb < 0 || sh_n[v] > sh_n[vb])) vb = v; if (vb >= 0 && sh_n[vb] > 2) --sh_n[vb]; }
    int lo = 0;
    bool first = true;
    for (int v = 0; v < G2G_NVAR; ++v) if (sh_n[v]) { if (!first) lo += gap; first = false; sh_lo[v] = lo; lo += sh_n[v]; }
    shares = lo <= 32;
}

// ---- (c) the launches of a run -------------------------------------------------------------------------------------
// Publish intervals (sweep mode: how many steps a strip runs between two publishes of its progress).  Three rules, each measured
// for its kernels: they differ on purpose.
// v2 (8 lanes per cell).  A DP's critical path is columns + strips x (rows of a strip + interval): 32 steps when the strips outnumber
// the resident workgroups many times over (throughput bound, fewer fences), 8 / 4 when they do not (a window of g2g_refine: the batch
// is as slow as its longest pipeline; measured on batches of 1-16 full-size DPs with tools/latency_probe.py: 4 beats 16 by 14 % at
// 8 DPs, 2 gains nothing more), 16 for a rank's share of a sharded sweep (1/8 of the bench sweep: 180 ms against 195 with 32).
static inline int publish_interval_v2(int sweep, int cnt, int resident)
{
    return !sweep ? 0 : sweep >= 2 ? sweep : cnt <= 2 * resident ? 4 : cnt <= 4 * resident ? 8 : cnt <= 16 * resident ? 16 : 32;
}
// v3 / v3r (_hf, one lane per cell): at most 8 strips per CU count as resident, and there is no step at 8.
static inline int publish_interval_v3(int sweep, int cnt, int cus, int wpc)
{
    return !sweep ? 0 : sweep >= 2 ? sweep : cnt <= cus * std::min(wpc, 8) ? 4 : cnt < 4 * cus * std::min(wpc, 8) ? 16 : 32;
}
// v6 / v7 / v8 (sweep mode only): 4 while the strips fill at most a quarter of the resident slots.  V2_SWEEP >= 2 sets it.
static inline int publish_interval_strip(int v2_sweep, int cnt, int cus, int wpc)
{
    return v2_sweep >= 2 ? v2_sweep : 4 * cnt <= cus * wpc ? 4 : cnt < 4 * cus * wpc ? 16 : 32;   // (a power of 2)
}

struct Launch {
    int slot, cnt;
    int k;                          // launch stream / join event of the run (unless the slot has a CU share: then its stream)
    int cus;                        // CUs of its share, or all
    int grid, block; size_t lds;
    int cols, pint, pro_off;        // kernel arguments: columns of a tile (1 << 20: sweep mode), publish interval, staged chains' LDS offset
    size_t scratch_bytes;           // column-score scratch (0: the kernel gets none)
    int twin_dw; size_t twin_bytes; // v6: the twin image of the strips' dynamic lists
    bool after_hf;                  // v6: starts when the _hf (v3 / v3r) launches are done
};
static inline std::vector<Launch> launch_plan(const RunFacts &f, const ShareOut &sh)
{
    std::vector<Launch> plan;
    const int pro_off = plan_pro_off(f);
    const int T2 = f.v2_threads;
    for (int o = 0; o < G2G_NLAUNCH_ORDER; ++o) {
        const int slot = G2G_LAUNCH_ORDER[o];
        const G2GVariant &var = G2G_VARIANT[slot];
        const int cnt = f.cnt[slot];
        if (!cnt || var.fam == G2G_NONE) continue;
        if (variant_is_v3(slot) && f.only_var_set && f.only_var != variant_v3_index(slot)) continue;
        Launch l;
        l.slot = slot; l.cnt = cnt;
        l.k = (int) plan.size() % G2G_NVS;                    // every persistent launch of a run takes the next stream
        l.cus = sh.shares ? 8 * sh.n[slot] : f.ncu;
        l.block = 64; l.cols = 0; l.twin_dw = 0; l.twin_bytes = 0; l.after_hf = false;
        bool scratch = true;
        switch (var.fam) {
        case G2G_V2: {
            const int wpc = f.v2_wpc ? f.v2_wpc : 2048 / T2;  // workgroups per CU the grid provides (LDS decides how many are resident)
            l.grid = std::min(cnt, l.cus * wpc);
            l.block = T2; l.lds = f.lds2 + 4 * T2;
            l.cols = f.v2_sweep ? (1 << 20) : f.v2_cols;
            l.pint = publish_interval_v2(f.v2_sweep, cnt, l.cus * std::max(1, std::min(wpc, (int) (V2_LDS_MAX / (f.lds2 + 4 * (size_t) T2)))));
            l.pro_off = (pro_off && pro_off + f.pro_lds_bytes <= f.lds2) ? pro_off : 0;
            scratch = f.v2_sweep && !f.no_simblk;
            break; }
        case G2G_V3_LDS: case G2G_V3R: {
            const LdsFacts &LO = f.v3[variant_v3_index(slot)];
            const bool swp = var.rec == G2G_REC_HF && f.v3_sweep;      // the _hf variants run in sweep mode
            const int wpc = f.v3_wpc ? f.v3_wpc : clamp_wpc((size_t) LO.total, 16);     // resident tiles per CU (LDS-bound)
            l.grid = std::min(cnt, l.cus * wpc);
            l.lds = (size_t) LO.total;
            l.cols = swp ? (1 << 20) : f.v3_cols;
            l.pint = publish_interval_v3(swp ? f.v3_sweep : 0, cnt, l.cus, wpc);
            l.pro_off = (pro_off && pro_off + (int) f.pro_lds_bytes <= LO.svals) ? pro_off : 0;
            scratch = swp && !f.no_simblk;
            break; }
        case G2G_V6: {
            const LdsFacts &LO = f.v6[variant_v6_index(slot)];
            // The _pf launches start when the _hf launches are done.  A sweep is bound by throughput -- its time is the SUM of what the
            // launches take alone (_hf 133 ms + _pf 610 ms for the bench sweep; the two footprint classes of v6 together take what
            // they take one after the other) -- and side by side the two kernel shapes leave each other wave slots they cannot use
            // (v3r: two waves per SIMD, v6: a whole SIMD's registers): 769 -> 744 ms.  PARALLEL_HF=1: side by side as before.
            l.after_hf = !f.parallel_hf;
            const int wpc = f.v6_wpc ? f.v6_wpc : clamp_wpc((size_t) LO.total, 4);      // resident strips per CU (LDS-bound; the kernel takes a whole SIMD's registers: four at most)
            l.grid = std::min(cnt, l.cus * wpc);
            l.lds = (size_t) LO.total;
            l.pint = publish_interval_strip(f.v2_sweep, cnt, l.cus, wpc);
            l.pro_off = (pro_off && pro_off + (int) f.pro_lds_bytes <= LO.svals) ? pro_off : 0;
            // the twin image of the strips' dynamic lists (what does not fit their inline parts in LDS): two dwords per dword of rows
            l.twin_dw = 2 * (LO.black - LO.rows) / 4 + 64;
            l.twin_bytes = (size_t) l.grid * l.twin_dw * sizeof(unsigned);
            break; }
        default: {                                            // v7: DPunit strips (no gap state, no LDS to speak of); v8: DPunit_nv strips
            const int wpc = var.fam == G2G_V8 ? 4 : 16;       // (v8 holds its records' lengths in registers: one wave per SIMD)
            l.grid = std::min(cnt, l.cus * wpc);
            l.lds = 0;
            l.pint = publish_interval_strip(f.v2_sweep, cnt, l.cus, wpc);
            l.pro_off = 0;
            break; }
        }
        l.scratch_bytes = scratch ? (size_t) l.grid * f.simblk_bytes : 0;
        plan.push_back(l);
    }
    return plan;
}

// ---- (d) the report of a time-out ----------------------------------------------------------------------------------
struct TimeoutView {
    const int *x;                   // the wait header as read back: x[0] time-outs, x[1] first queue slot, x[4 ..] the first time-out's snapshot (g2g_wait_ge)
    const int *dump;                // the dump area (2 + dump_words x dump_strips words), or 0 when there is none
    int dump_words, dump_strips;
    int gen, n, fail_off;
    bool is_retry;
    double rt_ticks_per_ms;
    struct Lost { int i, kernel, rows, cols; };
    std::vector<Lost> lost;
};
static inline std::string timeout_report_text(const TimeoutView &t)
{
    char buf[6144];
    int o = 0;
    auto add = [&](const char *fmt, ...) { va_list ap; va_start(ap, fmt); if (o < (int) sizeof buf - 1) { const int w = vsnprintf(buf + o, sizeof buf - o, fmt, ap); if (w > 0) o += w; } va_end(ap); if (o > (int) sizeof buf - 1) o = (int) sizeof buf - 1; };
    const int *x = t.x;
    int kinds[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (const auto &l : t.lost) if (l.kernel >= 0 && l.kernel < 10) ++kinds[l.kernel];
    add("%d waits timed out (first: queue slot %d, gen %d, batch of %d DPs): re-running %zu DP(s) %s; by kernel (0 v1, 1 v2, 2 v3, 3 v3r, 6 v6, 7 v7, 8 v8):",
        x[0], x[1], t.gen, t.n, t.lost.size(), t.is_retry ? "on g2g_forward_kernel" : "(first on the ordinary kernels)");
    for (int k = 0; k < 10; ++k) if (kinds[k]) add(" %d x kernel %d", kinds[k], k);
    add("; the first:");
    for (size_t k = 0; k < t.lost.size() && k < 6; ++k) add(" %d(kernel %d, %d x %d)", t.lost[k].i, t.lost[k].kernel, t.lost[k].rows, t.lost[k].cols);
    add(". First time-out: DP %d, wanted gen %d col %d of word %d, saw gen %d col %d; the words at and below it (gen:col):",
        x[7] - t.fail_off, (x[4] >> 20) & 0x7FF, x[4] & 0xFFFFF, x[6], (x[5] >> 20) & 0x7FF, x[5] & 0xFFFFF);
    for (int k = 0; k < 8; ++k) add(" %d:%d", (x[8 + k] >> 20) & 0x7FF, x[8 + k] & 0xFFFFF);
    if (!(x[16] == 0x7fffffff || (x[16] == 0 && x[17] == 0))) add("; producer's heartbeat: step %d place %d, 50 us later step %d place %d", x[16], x[17], x[18], x[19]);
    add("; producer HW_ID %08x XCC %d, waiter HW_ID %08x XCC %d; waiters per XCC:", x[20], x[21] & 15, x[22], x[23] & 15);
    for (int k = 0; k < 8; ++k) add(" %d", x[24 + k] / 64);
    add("; their producers per XCC:");
    for (int k = 0; k < 8; ++k) add(" %d", x[32 + k] / 64);
    add("; by RMW %d:%d, loaded again %d:%d", (x[46] >> 20) & 0x7FF, x[46] & 0xFFFFF, (x[47] >> 20) & 0x7FF, x[47] & 0xFFFFF);
    add("; columns the producer's waves left at their last publish (v2 / v3 strips): %d %d %d %d", x[42], x[43], x[44], x[45]);
    {   // -DG2G_HEARTBEAT builds: (step, place) of up to four waves of a v2 / v3 producer, twice, 50 us apart (all zero otherwise)
        bool any = false;
        for (int k = 48; k < 64; ++k) if (x[k]) any = true;
        if (any) {
            add("; producer's waves (step:place, then 50 us later):");
            for (int w = 0; w < 4; ++w) add(" w%d %d:%d -> %d:%d", w, x[48 + 2 * w], x[49 + 2 * w], x[56 + 2 * w], x[57 + 2 * w]);
        }
    }
    add("; the blocker (lowest strip of this DP without a publish in this generation, %d below the polled one): word %d:%d, HW_ID %08x XCC %08x, taken-by marker %08x (gen %d, workgroup %d), past the left chain %08x, past its first look at the strip above %08x, first wave's last publish %d (markers carry the generation; 7fffffff: never written)",
        x[64], (x[65] >> 20) & 0x7FF, x[65] & 0xFFFFF, x[66], x[67], x[68], (x[68] >> 20) & 0x7FF, x[68] & 0xFFFF, x[69], x[70], x[71]);
    if (t.dump && t.dump[0] > 0) {
        // the whole pipeline of the first time-out's DP as that waiter saw it: strips ti-1, ti-2, ... (word, HW_ID, markers, the
        // two waves' last publish).  A strip is TIGHT when its predecessor is less than 48 columns ahead (it can only be waiting
        // for it); the HEADS are the unfinished strips that are not tight: they wait for nobody's progress.
        const int *dump = t.dump;
        const int nd = std::min(dump[0], t.dump_strips), ti = dump[1];
        const int g1 = x[4] & ~0xFFFFF;
        auto colof = [&](int w) { return w < (g1 | 0) ? -1 : (w & 0xFFFFF); };      // -1: nothing in this generation
        int heads = 0, unfinished = 0, untaken = 0;
        add("; pipeline of that DP (%d strips above the waiter dumped): heads", nd);
        for (int k = 0; k < nd; ++k) {
            const int *d = dump + 2 + t.dump_words * k;
            const int c = colof(d[0]);
            if (c == 0xFFFFF) continue;
            ++unfinished;
            const bool taken = (d[2] & ~0xFFFFF) == (g1 | 0) || ((d[2] >> 20) & 0x7FF) == ((g1 >> 20) & 0x7FF);
            if (!taken) ++untaken;
            const int cp = k + 1 < nd ? colof(dump[2 + t.dump_words * (k + 1)]) : 0xFFFFF;      // predecessor (the top chain counts as finished)
            if (cp == 0xFFFFF || cp - c >= 48) {
                if (heads < 6) add(" [strip %d: col %d, predecessor %s%d, HW_ID %08x, taken %08x, past left chain %08x, past first look %08x, waves' last publish %d %d, waves' step:place %d:%d %d:%d]",
                                   ti - 1 - k, c, cp == 0xFFFFF ? "finished " : "col ", cp == 0xFFFFF ? 0 : cp, d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10]);
                ++heads;
            }
        }
        add(" -- %d head(s), %d unfinished strip(s), %d of them not taken from the queue in this generation", heads, unfinished, untaken);
    }
    add("; chain words of this DP as the first waiter saw them (valid when the polled word is a strip's): left %d:%d, top %d:%d", (x[80] >> 20) & 0x7FF, x[80] & 0xFFFFF, (x[81] >> 20) & 0x7FF, x[81] & 0xFFFFF);
    if (x[72]) add("; of the waves released when their DP was given up, the one with the lowest strip index (%d) was waiting on word %d for %d:%d and had last seen %d:%d (read-modify-write on release: %d:%d) after %d polls, %.0f ms of its own running time",
                   0x7fffffff - x[72], x[75], (x[73] >> 20) & 0x7FF, x[73] & 0xFFFFF, (x[74] >> 20) & 0x7FF, x[74] & 0xFFFFF, (x[78] >> 20) & 0x7FF, x[78] & 0xFFFFF, x[76], x[77] * 65536. / t.rt_ticks_per_ms);
    add("; waiting waves off the machine for > 4 ms at a stretch in this run: %d (longest %.1f ms)", x[40], x[41] * 1024. / t.rt_ticks_per_ms);
    buf[o] = 0;
    return buf;
}

// ---- (e) the LDS plan of a v6 launch -------------------------------------------------------------------------------
// Ring rows of dynamic lists, black lists, staging scalars, the rings of b's static lists, queue scratch, sinks (V6Lds and
// the window constants: g2g_lds.h).
// A ring is indexed by COMPACT pool position (pool position minus the terminators in front of it) modulo its size S.  S is the
// need of the DP -- the most list entries any V6_WINDOW consecutive columns of b hold -- rounded up to 32 entries, not to a
// power of two: the kernel reduces a position with a wave-uniform base and one conditional subtract (no mask, no division), and a
// MIRRORED TAIL of T entries behind the S (a copy of slots [0, T)) lets it read a list that starts at slot p < S as ring[p + k]
// without a wrap, for every k a merge loop asks for: k runs up to the wave's longest list, so T is the longest list of any view
// plus one, rounded up to 4.
struct V6Ring {
    int rs[3];                      // ring entries per view (s, t; r: V6_RHCOLS head freqs, one per column, no ring)
    int tail;                       // entries of the mirrored tail
    int need[3];                    // what rs was rounded up from
};
// off[v]: the offset table of view v of b's static lists (column c's list is [off[v][c + 1], off[v][c + 2]), terminator included)
static inline V6Ring v6_ring_need(const int32_t *const off[3], int left, int right)
{
    V6Ring R;
    int longest = 0;
    for (int v = 0; v < 3; ++v) {
        int need = 1;
        for (int c = left; c < right; ++c) {
            const int e = std::min(c + V6_WINDOW, right);
            need = std::max(need, (off[v][e + 1] - (e + 1)) - (off[v][c + 1] - (c + 1)));
            longest = std::max(longest, off[v][c + 2] - off[v][c + 1] - 1);
        }
        R.need[v] = need;
        R.rs[v] = v < 2 ? std::max(32, (need + 31) & ~31) : V6_RHCOLS;
    }
    R.tail = (longest + 1 + 3) & ~3;
    return R;
}
// the plan of a launch: the largest S per view and the largest T of its DPs, each taken separately
static inline void v6_ring_max(V6Ring &into, const V6Ring &r)
{
    for (int v = 0; v < 3; ++v) { into.rs[v] = std::max(into.rs[v], r.rs[v]); into.need[v] = std::max(into.need[v], r.need[v]); }
    into.tail = std::max(into.tail, r.tail);
}
static inline V6Lds v6_layout(int rows_bytes, int ca4max, const V6Ring &R)
{
    V6Lds L;
    int o = 0;
    auto take = [&](int bytes) { int r = o; o = (o + bytes + 15) & ~15; return r; };
    L.rows = take(rows_bytes);
    L.black = take(4 * (ca4max + 8));
    L.stsc = take(4 * 28);
    L.rtail = R.tail;
    for (int v = 0; v < 3; ++v) { L.rs[v] = R.rs[v]; L.ringf[v] = take(8 * (R.rs[v] + (v < 2 ? R.tail : 0))); }
    for (int v = 0; v < 3; ++v) L.ringk[v] = take(v < 2 ? 4 * (R.rs[v] + R.tail) : 0);      // (view 2: an array of head freqs per column, no keys)
    L.svals = take(4 * 64);
    L.sink = take(4 * 64 + 16 * 64);
    L.total = o;
    return L;
}
static inline int v6_rows_bytes(int capa, int capb, int noll)
{
    const int lsz = v6_inline_dw((capa + 3) & ~3) + v6_inline_dw((capb + 3) & ~3);      // the INLINE parts of a record's two lists (LS6)
    return 65 * v3_pitch(noll == 3 ? 9 : 6, lsz) * 4 + 32;
}
// A launch has ONE LDS plan, the largest of its DPs, and LDS decides how many strips a CU holds (the kernel takes a whole SIMD's
// registers: four per CU at most).  Class A (up to 40 KB, four strips per CU) is the default limit of v6: with a larger plan in
// the launch every strip of it drops to three per CU, and in a launch of their own the large DPs are bound by their critical
// path (measured when rings were powers of two: the bench sweep took 709-738 ms with limits of 46-49 KB against 660 ms at 40 KB).
// With rings of the size the lists need (and a window of 88 columns) every _pf DP of the bench sweep fits class A -- the 16
// balanced divisions whose 513-807 t entries used to take a 1024-entry ring and ran on the 8-lanes-per-cell kernel for it
// included (37-40 KB now; the rest of the sweep: up to 35 KB).  Classes B (up to V6_SMALL_KB) and C (V6_LARGE_KB) stay as
// options for measurements.
static const int V6_CLASS_A = 40 * 1024;

// ---- (f) prepare: what a batch's DPs are, the shape of the batch, the kernel of each DP ---------------------------------
// Every option g2g_batch_prepare reads, read once (prep_options in g2g_engine.hip).
struct PrepOptions {
    int ncu;
    bool force_v1, no_v7, no_v8, force_v2, no_v6, no_areg, no_strip_bonus, no_chainq, no_simblk;
    int v6_small, v6_large;         // V6_SMALL_KB / V6_LARGE_KB in bytes: the limits of footprint classes B and C (40 KB and none when not set)
    int v2_threads, v2_cols, v3_cols;           // V2_THREADS / V2_COLS / V3_COLS (0: not set)
    bool min_strips_set; long long min_strips;  // V6_MIN_STRIPS
    int v3_sweep, v2_sweep;         // V3_SWEEP / V2_SWEEP (1 when not set)
    bool inject; int inject_victim; // INJECT_STALL (test hook)
};
static inline PrepOptions prep_defaults(int ncu)
{
    PrepOptions o = {ncu, false, false, false, false, false, false, false, false, false, 40 * 1024, 0, 0, 0, 0, false, 0, 1, 1, false, 0};
    return o;
}
// What the decisions need of one DP (filled once per DP, after its sides were packed).
struct SideFacts {
    int len, many, left, right, nelm, felm;
    int maxlist, r_from_t;          // DevSide's (0 for a side whose gap profiles the DP does not read)
    bool gapdens, postgapdens, weight;          // the array is there
    const int32_t *off[3];          // gfq.off of the three views
};
struct DpFacts {
    int kind;                       // DevProb::kind (-1: not a valid problem)
    int rect, noll, capa, capb, nbonus, crg2_kind, sim2_kind, lw, up;
    SideFacts a, b;
};
struct BatchShape { int v3_cols, v2_threads, v2_cols; bool v6_on; int v3_sweep, v2_sweep; };
#define G2G_PLAN_V2_TILE_COLS 512   // G2G_V2_TILE_COLS of the build flags (the engine asserts that they agree)

// Tile widths.  Tiles of one DP run as a wavefront, at most min(strips, blocks) of them at a time: a sweep with
// hundreds of DPs fills the GPU with wide tiles (few block-boundary records, short fill/drain share), a rank
// that holds few DPs (the 8-GPU shard) needs narrow ones or its waves sit idle behind the dependencies.
static inline BatchShape batch_shape(const DpFacts *facts, int n, const PrepOptions &o)
{
    BatchShape s;
    const int ncu = o.ncu;
    auto pick = [&](int kind, int R, int cmax, int cmin, int slots) {
        int C = cmax;
        for (; C > cmin; C /= 2) {
            long long par = 0;
            for (int i = 0; i < n; ++i) {
                const DpFacts &d = facts[i];
                if (d.kind != kind) continue;
                const int ns = (d.a.right - d.a.left + R - 1) / R, nb = (d.b.right - d.b.left + C - 1) / C;
                par += std::min(ns, nb);
            }
            if (4 * par >= 5 * (long long) slots) break;
        }
        return C;
    };
    s.v3_cols = pick(1, 64, 128, 32, ncu * 4);
    // v2 (_pf): 16-row strips in 2-wave workgroups when the batch offers enough tiles (less barrier idling, 7 % faster
    // on a full sweep), 32-row strips otherwise (half as many strips on a DP's critical path)
    s.v2_threads = 128;
    if (pick(2, 16, 128, 64, ncu * 6) != 128) s.v2_threads = 256;      // (measured crossover: between 1/4 and 1/8 of the bench sweep)
    if (o.v2_threads == 128 || o.v2_threads == 256) s.v2_threads = o.v2_threads;
    s.v2_cols = pick(2, s.v2_threads / 8, G2G_PLAN_V2_TILE_COLS, 64, ncu * (768 / s.v2_threads));
    if (o.v2_cols >= 16 && o.v2_cols <= 4096) s.v2_cols = o.v2_cols;
    if (o.v3_cols >= 16 && o.v3_cols <= 4096) s.v3_cols = o.v3_cols;
    // v6 or v2 for the _pf DPs of this batch?  v6 has the higher throughput (a full sweep: 750 vs 800 ms) but the longer critical
    // path per DP (64-row strips at one wave per SIMD, ~19 us per step): a batch that cannot fill the machine -- a rank's share of
    // a sharded sweep -- finishes sooner on v2's 16-row strips.  Measured on shares of the bench sweep (v6 / v2, ms): 1/2 436 / 456,
    // 1/3 405 / 311, 1/4 327 / 254, 1/8 283 / 163.  Threshold: 35 strips of 64 rows per CU (between the 1/2 and the 1/3 share).
    long long s6 = 0;
    for (int i = 0; i < n; ++i) if (facts[i].kind == 2) s6 += (facts[i].a.right - facts[i].a.left + 63) / 64;
    s.v6_on = s6 >= (o.min_strips_set ? o.min_strips : 35LL * ncu);
    s.v3_sweep = o.v3_sweep;
    s.v2_sweep = o.v2_sweep;
    return s;
}

// bytes of a strip-boundary record in HBM and in the staging slots: v8 fixed, else 16 + the dynamic lists' entries, in 16-byte units
static inline size_t strip_record_bytes(int generation, int kind, int capa, int capb)
{
    return generation == G2G_V8 ? 4 * V8_REC : (16 + 4 * (size_t) (capa + (kind == 2 ? capb : 0)) + 15) & ~(size_t) 15;
}
// LDS footprint of the 8-lanes-per-cell strips (v2) for one problem (see V2Geom): (slots * R + extras) records
static inline size_t v2_lds_bytes(int kind, int noll, int capa, int capb, int mla, int mlb, int threads)
{
    const size_t recsz = strip_record_bytes(G2G_V2, kind, capa, capb);
    const size_t R = threads / 8;
    const size_t lists = (size_t) 10 * 3 * (R * mla + (kind == 2 ? (R + 2) * mlb : 0)) + 8;   // glen i16 + freq f64
    return (((noll == 3 ? 9 : 6) * R + 5) * recsz + 16 * R + lists + 16 + 15) & ~(size_t) 15;
}
// (v2 caches static gap lengths as SIGNED 16-bit with negative = terminator: a gap run can be as long as the group has columns,
// so sides of 32768 columns or more are not eligible -- they stay on v3 / v1, which keep 32 bits)
static inline bool v2_fits(const DpFacts &d, int threads)
{
    return std::max(d.a.len, d.b.len) < 32768 && v2_lds_bytes(d.kind, d.noll, d.capa, d.capb, d.a.maxlist, d.b.maxlist, threads) + 4 * threads <= V2_LDS_MAX;
}
// LDS plan of the v3 kernel (g2g_kernels_v3.hip) for one problem with C-column tiles: ring rows, the black
// list, staging scalars, and the static-list pools of a strip's rows / a block's columns
static inline V3Lds v3_layout(int rows_bytes, int ca4max, int apool, int bpool, int C)
{
    V3Lds L;
    int o = 0;
    auto take = [&](int bytes) { int r = o; o = (o + bytes + 15) & ~15; return r; };
    L.rows = take(rows_bytes);
    L.black = take(4 * (ca4max + 4));
    L.stsc = take(4 * 28);
    L.aglen = take(4 * (apool + 4));
    L.afreq = take(8 * (apool + 4));
    L.boff = take(bpool ? 4 * 3 * C : 0);
    L.bglen = take(bpool ? 4 * (bpool + 4) : 0);
    L.bfreq = take(bpool ? 8 * (bpool + 4) : 0);
    L.svals = take(4 * 64);
    L.sink = take(4 * 64);
    L.total = o;
    return L;
}
struct V3Need { int rows_bytes, ca4, apool, bpool, total; };
static inline V3Need v3_need(const DpFacts &d, int C, bool areg = false)
{
    V3Need n;
    const int capb = d.kind == 2 ? d.capb : 0;
    n.ca4 = (d.capa + 3) & ~3;
    const int lsz = n.ca4 + ((capb + 3) & ~3);
    n.rows_bytes = 65 * v3_pitch(d.noll == 3 ? 9 : 6, lsz) * 4;
    n.apool = 0; n.bpool = 0;
    const int al = d.a.left, ar = d.a.right, bl = d.b.left, br = d.b.right;
    for (int m0 = al; m0 < ar; m0 += 64) {
        const int me = std::min(m0 + 64, ar);
        int c = 0;
        for (int v = 0; v < 3; ++v) c += d.a.off[v][me + 1] - d.a.off[v][m0 + 1];
        n.apool = std::max(n.apool, c);
    }
    if (d.kind == 2)
        for (int c0 = bl; c0 < br; c0 += C) {
            const int c1 = std::min(c0 + C, br);
            int c = 0;
            for (int v = 0; v < 3; ++v) c += d.b.off[v][c1 + 1] - d.b.off[v][c0 + 1];
            n.bpool = std::max(n.bpool, c);
        }
    if (d.kind == 2 && !n.bpool) n.bpool = 1;
    if (areg) n.apool = 0;                                  // the rows' static lists live in registers
    n.total = v3_layout(n.rows_bytes, n.ca4, n.apool, n.bpool, C).total;
    return n;
}

// Which kernel generation runs a DP (DevProb::v2_ok): 0 g2g_forward_kernel, 1 v2, 2 v3 with LDS lists, 3 v3r, 6, 7, 8; ib: on a
// bonus-aware instantiation of it; for generation 6 the ring need of the DP and the total of its own LDS plan (its footprint class).
struct KernelChoice { int generation; char ib; int v6_total; V6Ring v6_ring; };
static inline KernelChoice choose_kernel(const DpFacts &d, const BatchShape &s, const PrepOptions &o, bool force_v1)
{
    KernelChoice k = {0, 0, 0, {{32, 32, V6_RHCOLS}, 4, {1, 1, 1}}};
    int gen = 0;
    const bool v1 = force_v1 || o.force_v1;
    if (d.kind == 0 && !d.rect && !v1 && !o.no_v7) gen = 7;      // DPunit: strips without gap state (the rectangular engine: g2g_forward_kernel)
    if (d.kind == 3 && !v1 && !o.no_v8) {
        // DPunit_nv: strips with the members' gap lengths in registers, for the member counts selAlnMode sends this way
        const int an = d.a.many, bn = d.b.many, ck = d.crg2_kind;
        const bool fits = ck == 11 ? (an == 1 && bn == 1) : (ck == 120 || ck == 121) ? (an == 1 && bn <= 5) :
                          (ck == 210 || ck == 211) ? (an <= 5 && bn == 1) : (ck == 220 || ck == 221) ? (an <= 3 && bn <= 3) : false;
        if (fits && d.a.gapdens && d.b.gapdens && d.a.postgapdens && d.b.postgapdens && (!(ck & 1) || ck == 11 || (d.a.weight && d.b.weight))) gen = 8;
    }
    if ((d.kind == 1 || d.kind == 2) && !v1 && d.a.len + d.b.len < 65000) {
        // _pf: one lane per cell with rank-form merges (v6) when the rows' static lists fit the register file
        bool v6 = s.v6_on && !o.force_v2 && !o.no_v6 && d.kind == 2 && d.a.maxlist <= (d.noll == 3 ? G2G_V6_NA3 : G2G_V6_NA) && d.a.r_from_t && d.b.r_from_t;
        if (v6) {
            k.v6_ring = v6_ring_need(d.b.off, d.b.left, d.b.right);
            k.v6_total = v6_layout(v6_rows_bytes(d.capa, d.capb, d.noll), (d.capa + 3) & ~3, k.v6_ring).total;
            v6 = k.v6_total <= std::max(o.v6_small, o.v6_large);
        }
        if (v6) gen = 6;
        else if (!o.force_v2 && !o.no_areg && d.kind == 1 && d.a.maxlist <= G2G_V3_NA && d.a.r_from_t && v3_need(d, s.v3_cols, true).total <= (int) V2_LDS_MAX) gen = 3;
        else {
            // lists too long for registers: the LDS-list one-lane-per-cell kernel, unless its LDS footprint leaves fewer than
            // three waves per CU and the 8-lanes-per-cell kernel fits (a 512 x 2048 nt DNA sweep with 17-32 entry lists and
            // Noll 3: 87 KB per strip; 28.3 s with it, 22.4 s on v2)
            const bool v2fit = v2_fits(d, s.v2_threads);
            const int v3tot = (!o.force_v2 && d.kind == 1) ? v3_need(d, s.v3_cols).total : (int) V2_LDS_MAX + 1;
            if (v3tot <= (int) V2_LDS_MAX && (v3tot <= (int) V2_LDS_MAX / 3 || !v2fit || o.no_areg)) gen = 2;
            else if (v2fit) gen = 1;
        }
    }
    if (d.nbonus) {
        // The intron-position bonus: g2g_forward_kernel (v1), and the bonus-aware instantiations of the strips without gap
        // state (v7), of the naive-record strips (v8) and of the 8-lanes-per-cell strips (v2, sweep mode) -- not v3 / v3r / v6
        // (register-bound), so an annotated _hf / _pf DP goes to v2 whatever would otherwise have claimed it, within v2's own
        // limits.  NO_STRIP_BONUS: v1 for all of them, as before the strips knew the bonus.
        const int was = gen;
        gen = 0;
        if (!o.no_strip_bonus) {
            if (was == 7 || was == 8) gen = was;
            else if (was >= 1 && was <= 6 && (d.kind == 1 || d.kind == 2) && s.v2_sweep && v2_fits(d, s.v2_threads)) gen = 1;
        }
        k.ib = gen ? 1 : 0;
    }
    k.generation = gen;
    return k;
}

#ifdef G2G_DEVICE_H_                // (diag_rows lives in g2g_device.h beside the descriptors, which are HIP types: the engine's units see it)
// in-band cells of a DP and its widest anti-diagonal (the stride of its trace)
struct BandCells { long long cells; int tstride; };
static inline BandCells band_cells(int al, int ar, int bl, int br, int lw, int up)
{
    BandCells r = {0, 1};
    for (int dd = al + bl; dd <= (ar - 1) + (br - 1); ++dd) {
        int mlo, mhi;
        diag_rows(dd, al, ar, bl, br, lw, up, &mlo, &mhi);
        const int c = mhi - mlo + 1;
        if (c > 0) r.cells += c;
        if (c > r.tstride) r.tstride = c;
    }
    return r;
}
#endif

// ---- (g) prepare: the queues of a batch ------------------------------------------------------------------------------------
// Tiles: (strip i of R rows) x (block j of C columns, C chosen per batch); per variant slot one queue ordered by wavefront i + j,
// headed by the boundary chains of its sweep-mode DPs; one completion flag per tile slot (empty slots count as done for ever).
// Everything g2g_batch_prepare uploads for the persistent kernels, and the LDS plans of the launches, as values.
struct QueuePlan {
    int bad;                        // index of a DP whose kernel has no variant slot (-1: none; nothing else is valid otherwise)
    std::vector<V2Tile> tiles;      // in upload order; slot v owns [var_off[v], var_off[v + 1])
    int var_off[G2G_NVAR + 1];
    long long var_cells[G2G_NVAR];  // in-band cells of the DPs of slot v
    std::vector<int> flags;         // the initial image of d_flags: queue heads, wait header, tile flags / progress words, then
    int fail_off, dump_off, xq_off; // ... the per-DP fail flags, the first time-out's dump area, the queue heads of the slots from G2G_PLAN_HDR on
    std::vector<int> ip;            // DPs whose boundary chains run in the prologue kernel (the others': as queue entries)
    size_t lds2p, simtile_lds;      // LDS of the prologue launch and of the tiled column-score kernel
    int v2_maxrows, v2_maxcols;     // longest a-range / b-range among the DPs on strips
    V3Lds v3lds[8];
    V6Lds v6lds[6];
    std::string v6_ring_plan;       // option V6_RING_PLAN: per v6 launch that has strips "<class x 2 + Noll 3>:<S of the s ring>,<S of the t ring>,<T>,<LDS bytes>", joined by ';'
};
static inline QueuePlan queue_plan(const DpFacts *facts, const KernelChoice *choice, const long long *cells, const BatchShape &s, const PrepOptions &o, int n)
{
    QueuePlan Q;
    Q.bad = -1; Q.lds2p = 0; Q.simtile_lds = 0; Q.v2_maxrows = 1; Q.v2_maxcols = 1; Q.fail_off = Q.dump_off = Q.xq_off = 0;
    for (int v = 0; v < G2G_NVAR; ++v) Q.var_cells[v] = 0;
    for (int v = 0; v <= G2G_NVAR; ++v) Q.var_off[v] = 0;
    std::vector<std::vector<std::vector<V2Tile> > > q(G2G_NVAR);  // [variant][wavefront] -> tiles
    std::vector<int> &flags = Q.flags;
    flags.assign(G2G_PLAN_HDR + G2G_HDRN, 0);         // queue heads, then the header of the waits (g2g_wait_ge)
    std::vector<V2Tile> pre[G2G_NVAR];                // boundary chains of sweep-mode DPs: they head their variant's queue
    int v6rows[6] = {0, 0, 0, 0, 0, 0}, v6ca4[6] = {0, 0, 0, 0, 0, 0};
    V6Ring v6rs[6];
    for (int v = 0; v < 6; ++v) { const V6Ring r0 = {{32, 32, V6_RHCOLS}, 4, {1, 1, 1}}; v6rs[v] = r0; }
    V3Need need[8];
    for (int v = 0; v < 8; ++v) { const V3Need z = {0, 0, 0, 0, 0}; need[v] = z; }
    for (int i = 0; i < n; ++i) {
        const DpFacts &d = facts[i];
        const int gen = choice[i].generation;
        if (d.kind < 0 || !gen) continue;
        Q.lds2p = std::max(Q.lds2p, 5 * strip_record_bytes(gen, d.kind, d.capa, d.capb) + 64);
        Q.v2_maxrows = std::max(Q.v2_maxrows, d.a.right - d.a.left);
        Q.v2_maxcols = std::max(Q.v2_maxcols, d.b.right - d.b.left);
        if (d.a.nelm > 0 && sim_tiled_kind(d.sim2_kind)) {        // a's profile rows + b's frequency vectors or residues
            const bool vecb = d.sim2_kind == 33 || d.sim2_kind == 330;
            Q.simtile_lds = std::max(Q.simtile_lds, (size_t) 8 * SIM_TR * ((d.a.nelm - d.a.felm + 1) & ~1) + (vecb ? (size_t) 8 * SIM_TC * (d.b.felm > 0 ? d.b.felm : 0) : (size_t) SIM_TC * d.b.many) + 64);
        }
        const int al = d.a.left, ar = d.a.right, bl_ = d.b.left, br = d.b.right;
        const int R = gen >= 2 ? 64 : s.v2_threads / 8;
        const bool swp3 = (gen == 3 || gen == 2) && d.kind == 1 && s.v3_sweep;   // one tile per strip, pipelined (kind 1 only: no column pool)
        const bool swp2 = (gen == 1 && s.v2_sweep) || gen >= 6;      // (v6 and v7 know sweep mode only)
        const int C = (swp3 || swp2) ? (1 << 20) : gen >= 2 ? s.v3_cols : s.v2_cols;
        const int nstrip = (ar - al + R - 1) / R, nblk = (br - bl_ + C - 1) / C;
        // (one LDS plan per launch = the largest of its DPs: DPs whose column lists need a big ring get a launch of their own,
        //  or a handful of balanced divisions would cost every strip of the sweep its occupancy)
        const int v6fp = gen != 6 ? 0 : choice[i].v6_total > o.v6_small ? 2 : choice[i].v6_total > V6_CLASS_A ? 1 : 0;      // footprint class A / B / C
        const int var = variant_slot(gen, d.kind, d.noll, choice[i].ib != 0, v6fp);
        if (var < 0) { Q.bad = i; return Q; }
        Q.var_cells[var] += cells[i];
        if (gen == 6) {
            const int v6cls = variant_v6_index(var);
            v6rows[v6cls] = std::max(v6rows[v6cls], v6_rows_bytes(d.capa, d.capb, d.noll));
            v6ca4[v6cls] = std::max(v6ca4[v6cls], (d.capa + 3) & ~3);
            v6_ring_max(v6rs[v6cls], choice[i].v6_ring);
        } else if (gen >= 2 && gen < 7) {
            const V3Need nd = v3_need(d, C, gen == 3);
            V3Need &x = need[variant_v3_index(var)];
            x.rows_bytes = std::max(x.rows_bytes, nd.rows_bytes); x.ca4 = std::max(x.ca4, nd.ca4);
            x.apool = std::max(x.apool, nd.apool); x.bpool = std::max(x.bpool, nd.bpool);
        }
        const bool cq = (!o.no_chainq && (swp2 || swp3)) || gen >= 7;      // (v7's and v8's chains always run as queue entries: the prologue kernel knows the gap-profile kinds only)
        int ftop = -1, fleft = -1;
        if (cq) {
            ftop = (int) flags.size(); fleft = ftop + G2G_FSTRIDE;
            flags.resize(flags.size() + 2 * G2G_FSTRIDE, 0);
            V2Tile T;
            T.prob = i; T.tj = 0; T.nsteps = 0; T.dep_up = T.dep_left = T.dep_diag = T.dep_war = -1;
            T.ti = -1; T.self = ftop; pre[var].push_back(T);
            T.ti = -2; T.self = fleft; pre[var].push_back(T);
        } else Q.ip.push_back(i);
        const int fbase = (int) flags.size();
        flags.resize(flags.size() + (size_t) nstrip * nblk * G2G_FSTRIDE, 0x7fffffff);
        for (int ti = 0; ti < nstrip; ++ti) {
            const int m0 = al + ti * R;
            for (int tj = 0; tj < nblk; ++tj) {
                const int c0 = bl_ + tj * C, c1 = std::min(c0 + C, br);
                const int cbase = std::max(std::max(m0 + d.lw, bl_), c0);
                int nsteps = 0;
                for (int t = 0; t < R && m0 + t < ar; ++t) {
                    const int m = m0 + t;
                    const int lo = std::max(std::max(m + d.lw, bl_), c0), hi = std::min(std::min(m + d.up + 1, br), c1);
                    if (hi > lo) nsteps = std::max(nsteps, hi - cbase + t);
                }
                if (!nsteps) continue;
                V2Tile T;
                T.prob = i; T.ti = ti; T.tj = tj; T.nsteps = nsteps;
                T.self = fbase + (ti * nblk + tj) * G2G_FSTRIDE;
                T.dep_up = ti > 0 ? T.self - nblk * G2G_FSTRIDE : ftop;             // sweep mode: the top chain is strip 0's "strip above"
                T.dep_left = tj > 0 ? T.self - G2G_FSTRIDE : fleft;
                T.dep_diag = (ti > 0 && tj > 0) ? T.self - (nblk + 1) * G2G_FSTRIDE : -1;
                T.dep_war = (ti > 1 && tj + 1 < nblk) ? T.self - (2 * nblk - 1) * G2G_FSTRIDE : -1;
                flags[T.self] = 0;
                const int k = ti + tj;
                if ((int) q[var].size() <= k) q[var].resize(k + 1);
                q[var][k].push_back(T);
            }
        }
    }
    std::vector<V2Tile> &all = Q.tiles;
    for (int v = 0; v < G2G_NVAR; ++v) {
        Q.var_off[v] = (int) all.size();
        all.insert(all.end(), pre[v].begin(), pre[v].end());
        for (size_t k = 0; k < q[v].size(); ++k) all.insert(all.end(), q[v][k].begin(), q[v][k].end());
    }
    Q.var_off[G2G_NVAR] = (int) all.size();
    for (int v = 0; v < 6; ++v) Q.v6lds[v] = v6_layout(v6rows[v], v6ca4[v], v6rs[v]);
    for (int sl = 0; sl < G2G_NVAR; ++sl) {
        const int v = variant_v6_index(sl);
        if (v < 0 || Q.var_off[sl + 1] == Q.var_off[sl]) continue;
        char buf[96];
        snprintf(buf, sizeof buf, "%s%d:%d,%d,%d,%d", Q.v6_ring_plan.empty() ? "" : ";", v, Q.v6lds[v].rs[0], Q.v6lds[v].rs[1], Q.v6lds[v].rtail, Q.v6lds[v].total);
        Q.v6_ring_plan += buf;
    }
    for (int v = 0; v < 8; ++v) Q.v3lds[v] = v3_layout(need[v].rows_bytes, need[v].ca4, need[v].apool, need[v].bpool, s.v3_cols);
    // test hook: INJECT_STALL=<i> makes the first strip / tile of problem i depend on a flag nobody ever writes
    if (o.inject) {
        const int never = (int) flags.size();
        flags.resize(flags.size() + G2G_FSTRIDE, 0);
        for (size_t k = 0; k < all.size(); ++k)
            if (all[k].prob == o.inject_victim && all[k].ti >= 0) { all[k].dep_up = never; break; }
    }
    Q.fail_off = (int) flags.size();                  // per-DP fail flags behind the tile flags
    flags.resize(flags.size() + (size_t) (n > 0 ? n : 1), 0);
    Q.dump_off = (int) flags.size();                  // the first time-out's view of its whole DP (g2g_wait_ge: G2G_DUMP_STRIPS strips x G2G_DUMP_WORDS words)
    flags.resize(flags.size() + 2 + G2G_DUMP_WORDS * G2G_DUMP_STRIPS, 0);
    Q.xq_off = (int) flags.size();                    // queue heads of the bonus-aware variants
    flags.resize(flags.size() + (G2G_NVAR - G2G_PLAN_HDR), 0);
    return Q;
}
#endif
