// plan_main.cc -- runs the host-side planning of prrn_aln_amd/csrc/g2g_plan.h over a fixed list of cases and prints one line
// per result (tests/test_host_plan.py compares the output with tests/golden/host_plan/*.txt).  No GPU, no HIP.
//   plan_main slots | shares | launches | report | choose | shape | queues
#include <string.h>
#include "g2g_plan.h"

// ---- variant_slot: every combination, holes included ----
static void run_slots()
{
    const int gens[] = {0, 1, 2, 3, 6, 7, 8};
    for (int g : gens) for (int kind = 0; kind < 4; ++kind) for (int noll = 2; noll <= 3; ++noll) for (int ib = 0; ib < 2; ++ib) for (int cls = 0; cls < 3; ++cls)
        printf("generation %d kind %d noll %d ib %d class %d -> slot %d\n", g, kind, noll, ib, cls, variant_slot(g, kind, noll, ib != 0, cls));
    for (int s = 0; s < G2G_NVAR; ++s) {
        const G2GVariant &r = G2G_VARIANT[s];
        if (r.fam == G2G_NONE) { printf("slot %d: no kernel\n", s); continue; }
        printf("slot %d: %s family %d record %d noll3 %d ib %d class %d cost %.2f v3 index %d v6 index %d path %d\n", s, r.name, (int) r.fam, (int) r.rec,
               r.noll3 ? 1 : 0, r.ib ? 1 : 0, r.cls, variant_cost(s), variant_v3_index(s), variant_v6_index(s), family_path((int) r.fam));
    }
    printf("launch order:");
    for (int o = 0; o < G2G_NLAUNCH_ORDER; ++o) printf(" %d", G2G_LAUNCH_ORDER[o]);
    printf("\n");
}

// ---- cu_share_plan ----
static ShareIn share_base()
{
    ShareIn in;
    for (int v = 0; v < G2G_NVAR; ++v) { in.cnt[v] = 0; in.cells[v] = 0; in.wpc[v] = 1; }
    in.ncu = 256; in.mode_set = false; in.mode = 0; in.debug = false; in.no_share_gap = false; in.mstream_cap = 8;
    return in;
}
static void put(ShareIn &in, int slot, int cnt, long long cells, int wpc) { in.cnt[slot] = cnt; in.cells[slot] = cells; in.wpc[slot] = wpc; }
static void show(const char *name, const ShareIn &in)
{
    ShareOut out;
    cu_share_plan(in, out);
    printf("%s: shares %d", name, out.shares ? 1 : 0);
    if (out.shares) for (int v = 0; v < G2G_NVAR; ++v) if (out.n[v]) printf(" slot %d: %d..%d", v, out.lo[v], out.lo[v] + out.n[v] - 1);
    printf("\n");
}
static ShareIn window2()                       // a window of a refinement: _pf on v2 (three workgroups per CU) beside _hf on v3r
{
    ShareIn in = share_base();
    put(in, 2, 1400, 90000000LL, 3); put(in, 8, 700, 60000000LL, 10);
    return in;
}
static void run_shares()
{
    { ShareIn in = window2(); show("window, no stream alive", in); in.no_share_gap = true; show("window, NO_SHARE_GAP", in); }
    for (int gapless = 0; gapless < 2; ++gapless) {
        ShareIn in = window2(); in.no_share_gap = gapless != 0;
        const char *g = gapless ? " (NO_SHARE_GAP)" : "";
        char name[96];
        in.alive.clear(); in.alive.push_back(std::make_pair(0, 27)); in.alive.push_back(std::make_pair(27, 5));
        snprintf(name, sizeof name, "window, a pair one unit off alive%s", g); show(name, in);
        in.alive.clear(); in.alive.push_back(std::make_pair(0, 23)); in.alive.push_back(std::make_pair(23, 9));
        snprintf(name, sizeof name, "window, a pair five units off alive, under the cap%s", g); show(name, in);
        in.mstream_cap = 3;
        snprintf(name, sizeof name, "window, a pair five units off alive, at the cap%s", g); show(name, in);
        in.mstream_cap = 8; in.alive.clear(); in.alive.push_back(std::make_pair(0, 27));
        snprintf(name, sizeof name, "window, a stream without its partner alive%s", g); show(name, in);
    }
    { ShareIn in = share_base(); in.mode_set = true; in.mode = 2; put(in, 2, 1400, 90000000LL, 3); put(in, 8, 700, 60000000LL, 10); put(in, 16, 900, 40000000LL, 16); show("three launches, mode 2", in); }
    { ShareIn in = share_base(); in.mode_set = true; in.mode = 2; put(in, 0, 800, 50000000LL, 3); put(in, 2, 1400, 90000000LL, 3); put(in, 8, 700, 60000000LL, 10); put(in, 9, 300, 20000000LL, 8); show("four launches, mode 2", in); }
    { ShareIn in = share_base(); in.mode_set = true; in.mode = 2; put(in, 2, 1400, 90000000LL, 3); put(in, 8, 10, 60000000LL, 10); put(in, 16, 900, 40000000LL, 16); show("a launch of 10 tiles capped, the rest re-divided", in); }
    {
        ShareIn in = share_base(); in.mode_set = true; in.mode = 2;
        const int s[8] = {0, 1, 2, 3, 4, 5, 8, 9};
        for (int k = 0; k < 8; ++k) put(in, s[k], 5000, 1000, 3);
        in.cells[8] = 2500000LL;                  // slot 8 costs 1.0 per cell: about 1000 times the work of each of the others
        show("eight launches, work 1000 : 1 : ... : 1 (the minimum of one unit each overdrew)", in);
    }
    { ShareIn in = window2(); in.ncu = 304; show("refused: 304 CUs", in); }
    { ShareIn in = share_base(); put(in, 2, 1400, 90000000LL, 3); show("refused: one launch", in); }
    { ShareIn in = share_base(); in.mstream_cap = 2; put(in, 2, 1400, 90000000LL, 3); put(in, 8, 700, 60000000LL, 10); put(in, 16, 900, 40000000LL, 16); show("refused: three launches, MSTREAM_MAX 2", in); }
    { ShareIn in = window2(); in.mode_set = true; in.mode = 0; show("refused: mode 0", in); }
    { ShareIn in = window2(); put(in, 12, 500, 70000000LL, 4); show("refused: mode unset, a v6 slot not empty", in); in.mode_set = true; in.mode = 2; show("mode 2, a v6 slot not empty", in); }
    { ShareIn in = share_base(); in.mode_set = true; in.mode = 1; put(in, 2, 600, 90000000LL, 3); put(in, 8, 700, 60000000LL, 10); show("refused: mode 1, demand below twice the CUs", in); put(in, 2, 1400, 90000000LL, 3); show("mode 1, demand above twice the CUs", in); }
    { ShareIn in = window2(); in.debug = true; show("refused: DEBUG", in); }
}

// ---- launch_plan ----
static RunFacts facts_base()
{
    RunFacts f;
    for (int v = 0; v < G2G_NVAR; ++v) { f.cnt[v] = 0; f.cells[v] = 0; }
    f.ncu = 256; f.lds2 = 50000; f.lds2p = 2000;
    f.v2_threads = 256; f.v2_sweep = 1; f.v3_sweep = 1; f.v2_cols = 512; f.v3_cols = 128;
    for (int k = 0; k < 8; ++k) { const LdsFacts x = {20000 + 16 * k, 19000 + 16 * k, 0, 15000 + 16 * k}; f.v3[k] = x; }
    for (int k = 0; k < 6; ++k) { const LdsFacts x = {30000 + 12000 * (k / 2), 29000 + 12000 * (k / 2), 0, 24000 + 10000 * (k / 2) + 64 * k}; f.v6[k] = x; }
    f.v2_wpc = f.v3_wpc = f.v6_wpc = 0; f.only_var_set = false; f.only_var = 0;
    f.no_simblk = f.no_prostage = f.parallel_hf = false;
    f.pro_lds_bytes = 14352; f.simblk_bytes = 3 * 4096 * 8;
    return f;
}
static ShareOut no_shares() { ShareOut s; s.shares = false; for (int v = 0; v < G2G_NVAR; ++v) { s.lo[v] = 0; s.n[v] = 0; } return s; }
static void show(const char *name, const RunFacts &f, const ShareOut &sh)
{
    const std::vector<Launch> plan = launch_plan(f, sh);
    printf("%s: %zu launch(es)\n", name, plan.size());
    for (size_t i = 0; i < plan.size(); ++i) {
        const Launch &l = plan[i];
        printf("  slot %d (%s) %d entries: stream %d, %d CUs, grid %d x %d, lds %zu, cols %d, publish %d, pro_off %d, scratch %zu, twin %d dw / %zu bytes, waits for _hf:",
               l.slot, G2G_VARIANT[l.slot].name, l.cnt, l.k, l.cus, l.grid, l.block, l.lds, l.cols, l.pint, l.pro_off, l.scratch_bytes, l.twin_dw, l.twin_bytes);
        if (l.after_hf) for (size_t j = 0; j < i; ++j) if (variant_is_v3(plan[j].slot)) printf(" %d", plan[j].k);
        printf("\n");
    }
}
static void show(const char *name, const RunFacts &f) { show(name, f, no_shares()); }
static RunFacts with(int s0, int c0, int s1 = -1, int c1 = 0, int s2 = -1, int c2 = 0, int s3 = -1, int c3 = 0)
{
    RunFacts f = facts_base();
    f.cnt[s0] = c0; if (s1 >= 0) f.cnt[s1] = c1; if (s2 >= 0) f.cnt[s2] = c2; if (s3 >= 0) f.cnt[s3] = c3;
    return f;
}
static RunFacts every_family()
{
    RunFacts f = facts_base();
    for (int v = 0; v < G2G_NVAR; ++v) if (G2G_VARIANT[v].fam != G2G_NONE) { f.cnt[v] = 300 + 170 * v; f.cells[v] = 1000000LL * (v + 3); }
    return f;
}
static void run_launches()
{
    for (int T = 128; T <= 256; T += 128) for (int sweep = 1; sweep >= 0; --sweep) {
        RunFacts f = with(0, 900, 3, 5000, 26, 40, 29, 2500);
        f.v2_threads = T; f.v2_sweep = sweep;
        char name[64];
        snprintf(name, sizeof name, "v2, %d threads, %s mode", T, sweep ? "sweep" : "tile");
        show(name, f);
    }
    show("v3 with LDS lists", with(4, 700, 5, 3000));
    { RunFacts f = with(4, 700, 5, 3000, 8, 900); f.v3_sweep = 0; show("v3 / v3r, tile mode", f); }
    show("v3r", with(8, 1200, 9, 20));
    show("v6 classes A and C, behind v3r", with(12, 4000, 13, 600, 20, 90, 8, 1000));
    { RunFacts f = with(16, 5000, 17, 30, 18, 2000, 19, 7); f.cnt[24] = 100; f.cnt[25] = 3; f.cnt[30] = 900; f.cnt[31] = 1; show("v7, v8 and their _ib", f); }
    show("every family", every_family());
    {
        const RunFacts f = every_family();
        ShareIn in = share_base();
        in.mode_set = true; in.mode = 2; in.mstream_cap = 64;
        for (int v = 0; v < G2G_NVAR; ++v) { in.cnt[v] = f.cnt[v]; in.cells[v] = f.cells[v]; in.wpc[v] = share_wpc(f, v); }
        ShareOut sh;
        cu_share_plan(in, sh);
        show("every family, with CU shares", f, sh);
        printf("share_wpc:");
        for (int v = 0; v < G2G_NVAR; ++v) if (G2G_VARIANT[v].fam != G2G_NONE) printf(" %d", share_wpc(f, v));
        printf("\n");
    }
    // both sides of every threshold of the three publish-interval rules
    {
        const int res2 = 256 * 3;                 // v2: 256 CUs x 3 resident workgroups (50000 + 1024 bytes of LDS each)
        const int t2[3] = {2 * res2, 4 * res2, 16 * res2};
        for (int k = 0; k < 3; ++k) for (int d = 0; d < 2; ++d) { char name[64]; snprintf(name, sizeof name, "v2 rule, %d strips", t2[k] + d); show(name, with(2, t2[k] + d)); }
        const int res3 = 256 * 8;                 // v3: 256 CUs x min(8 resident strips, 8)
        const int t3[2] = {res3, 4 * res3 - 1};
        for (int k = 0; k < 2; ++k) for (int d = 0; d < 2; ++d) { char name[64]; snprintf(name, sizeof name, "v3 rule, %d strips", t3[k] + d); show(name, with(8, t3[k] + d)); }
        const int slot[3] = {12, 16, 18}, wpc[3] = {4, 16, 4};      // v6, v7, v8
        for (int s = 0; s < 3; ++s) {
            const int ts[2] = {256 * wpc[s] / 4, 4 * 256 * wpc[s] - 1};
            for (int k = 0; k < 2; ++k) for (int d = 0; d < 2; ++d) { char name[64]; snprintf(name, sizeof name, "strip rule, slot %d, %d strips", slot[s], ts[k] + d); show(name, with(slot[s], ts[k] + d)); }
        }
    }
    { RunFacts f = with(0, 900, 3, 5000); f.v2_wpc = 2; show("V2_WPC=2", f); }
    { RunFacts f = with(4, 700, 8, 3000); f.v3_wpc = 3; show("V3_WPC=3", f); }
    { RunFacts f = with(12, 4000, 21, 600); f.v6_wpc = 2; show("V6_WPC=2", f); }
    { RunFacts f = with(4, 700, 5, 3000, 8, 900, 9, 20); f.cnt[2] = 100; f.only_var_set = true; f.only_var = 4; show("ONLY_VAR=4", f); }
    { RunFacts f = with(12, 4000, 13, 600, 20, 90, 8, 1000); f.parallel_hf = true; show("PARALLEL_HF", f); }
    { RunFacts f = with(0, 900, 8, 1200, 12, 4000); f.no_prostage = true; show("NO_PROSTAGE", f); }
    { RunFacts f = with(0, 900, 8, 1200, 12, 4000); f.lds2p = 40000; show("staged chains that do not fit", f); }
    { RunFacts f = with(2, 20000, 8, 1200, 12, 4000, 16, 5000); f.v2_sweep = 4; show("V2_SWEEP=4", f); }
    { RunFacts f = with(2, 20000, 8, 1200, 12, 4000, 16, 5000); f.no_simblk = true; show("NO_SIMBLK", f); }
}

// ---- timeout_report_text ----
static int word(int gen, int col) { return (gen << 20) | col; }
static void base_header(int *x, int gen)
{
    memset(x, 0, 104 * sizeof(int));
    x[0] = 3; x[1] = 2;
    x[4] = word(gen, 640); x[5] = word(gen, 512); x[6] = 9344; x[7] = 70005;
    for (int k = 0; k < 8; ++k) x[8 + k] = word(gen - (k > 5 ? 1 : 0), 512 + 64 * k);
    x[16] = 0x7fffffff;
    x[20] = 0x00a41203; x[21] = 0x35; x[22] = 0x00b40107; x[23] = 0x12;
    for (int k = 0; k < 8; ++k) { x[24 + k] = 64 * (k + 1); x[32 + k] = 64 * (8 - k); }
    x[40] = 0; x[41] = 0; x[42] = 500; x[43] = 501; x[44] = 0; x[45] = 0;
    x[46] = word(gen, 512); x[47] = word(gen, 513);
    x[64] = 3; x[65] = word(gen, 448); x[66] = 0x00a41203; x[67] = 5; x[68] = word(gen, 0) | 417; x[69] = word(gen, 1); x[70] = 0x7fffffff; x[71] = 448;
    x[80] = word(gen, 0xFFFFF); x[81] = word(gen, 0xFFFFF);
}
static void run_report()
{
    const int gen = 5, W = 11, S = 580;
    TimeoutView t;
    int x[104];
    t.x = x; t.dump = 0; t.dump_words = W; t.dump_strips = S;
    t.gen = gen; t.n = 102; t.fail_off = 70000; t.is_retry = false; t.rt_ticks_per_ms = 100000.;
    const TimeoutView::Lost l0 = {5, 1, 640, 1300}, l1 = {17, 3, 200, 1310}, l2 = {18, 1, 64, 90};
    t.lost.push_back(l0); t.lost.push_back(l1); t.lost.push_back(l2);
    base_header(x, gen);
    printf("no dump area: %s\n", timeout_report_text(t).c_str());

    std::vector<int> dump(2 + W * S, 0);
    const int nd = 6;
    dump[0] = nd; dump[1] = 9;                    // the waiter is strip 9; strips 8 .. 3 dumped
    const int cols[nd] = {512, 530, 900, 0xFFFFF, 100, 0xFFFFF};       // strip 8 tight behind 7; 7 a head; 6 a head (its predecessor finished); 4 a head
    for (int k = 0; k < nd; ++k) {
        int *d = dump.data() + 2 + W * k;
        d[0] = word(gen, cols[k]); d[1] = 0x00a41200 + k; d[2] = word(gen, 0) | (400 + k); d[3] = word(gen, 1); d[4] = word(gen, 2);
        d[5] = cols[k] - 3; d[6] = cols[k] - 2; d[7] = 70 + k; d[8] = 2; d[9] = 71 + k; d[10] = 3;
    }
    dump[2 + W * 4] = word(gen - 1, 100); dump[2 + W * 4 + 2] = word(gen - 1, 0) | 77;      // strip 4: nothing in this generation, not taken from the queue
    t.dump = dump.data();
    t.is_retry = true;
    printf("two heads and an untaken strip, a retry: %s\n", timeout_report_text(t).c_str());

    t.is_retry = false; t.dump = dump.data(); dump[0] = 0;                                    // (a dump area nobody filled)
    x[16] = 120; x[17] = 4; x[18] = 121; x[19] = 6;
    for (int w = 0; w < 4; ++w) { x[48 + 2 * w] = 100 + w; x[49 + 2 * w] = 1 + w; x[56 + 2 * w] = 101 + w; x[57 + 2 * w] = 2 + w; }
    x[40] = 2; x[41] = 900;
    x[72] = 0x7fffffff - 7; x[73] = word(gen, 700); x[74] = word(gen, 650); x[75] = 9408; x[76] = 123456; x[77] = 800; x[78] = word(gen, 651);
    for (int k = 0; k < 9; ++k) { const TimeoutView::Lost l = {30 + k, k < 4 ? 6 : k < 7 ? 7 : 0, 100 + k, 200 + k}; t.lost.push_back(l); }
    printf("heartbeats and a released waiter: %s\n", timeout_report_text(t).c_str());
}

// ---- prepare: choose_kernel, batch_shape, queue_plan ----
// Synthetic sides: offset tables built here (column c's list of view v is [off[v][c + 1], off[v][c + 2]), terminator included).
struct Tables {
    std::vector<int32_t> off[3];
    Tables(int len, int k0, int k1, int k2) { const int k[3] = {k0, k1, k2}; for (int v = 0; v < 3; ++v) { off[v].assign(len + 2, 0); for (int i = 1; i < len + 2; ++i) off[v][i] = off[v][i - 1] + k[v] + 1; } }
    void longer(int v, int col, int extra) { for (size_t i = col + 2; i < off[v].size(); ++i) off[v][i] += extra; }      // `extra` more entries in column col's list
};
static SideFacts side(const Tables &t, int len, int many, int maxlist)
{
    SideFacts s = {len, many, 0, len, 0, 0, maxlist, 1, false, false, false, {t.off[0].data(), t.off[1].data(), t.off[2].data()}};
    return s;
}
static DpFacts dp(int kind, int noll, const Tables &ta, int alen, const Tables &tb, int blen, int capa = 4, int capb = 4)
{
    DpFacts d;
    d.kind = kind; d.rect = 0; d.noll = noll; d.capa = capa; d.capb = kind == 2 || kind == 3 ? capb : 0; d.nbonus = 0; d.crg2_kind = 0; d.sim2_kind = 0;
    d.lw = -alen; d.up = blen;
    d.a = side(ta, alen, 4, kind == 1 || kind == 2 ? 3 : 0); d.b = side(tb, blen, 4, kind == 2 ? 3 : 0);
    if (kind != 2) d.b.r_from_t = 0;
    if (kind == 0 || kind == 3) d.a.r_from_t = 0;
    return d;
}
static BatchShape shape_base() { const BatchShape s = {128, 256, 512, true, 1, 1}; return s; }
static void show(const char *name, const DpFacts &d, const BatchShape &s, const PrepOptions &o, bool force_v1 = false)
{
    const KernelChoice k = choose_kernel(d, s, o, force_v1);
    printf("%s: generation %d ib %d", name, k.generation, (int) k.ib);
    if (k.generation == 6) printf(" v6 total %d class %d", k.v6_total, k.v6_total > o.v6_small ? 2 : k.v6_total > V6_CLASS_A ? 1 : 0);
    printf("\n");
}
// a _pf DP whose own v6 plan has the fewest bytes in [lo, hi]: list capacities and b's list lengths are searched
struct Found { int capa, capb, k0, k1, extra, total; };
static Found find_v6(int noll, int lo, int hi)
{
    struct Ring { int k0, k1, extra; V6Ring r; };
    static std::vector<Ring> rings;               // the ring needs of b's candidate tables, walked once
    if (rings.empty())
        for (int k0 = 0; k0 <= 12; ++k0) for (int k1 = 0; k1 <= 12; ++k1) for (int extra = 0; extra <= 60; extra += 4) {
            Tables tb(300, k0, k1, k1 + 1); tb.longer(1, 150, extra);
            const int32_t *off[3] = {tb.off[0].data(), tb.off[1].data(), tb.off[2].data()};
            const Ring r = {k0, k1, extra, v6_ring_need(off, 0, 300)};
            rings.push_back(r);
        }
    Found best = {0, 0, 0, 0, 0, hi + 1};
    for (int capa = 1; capa <= 40 && best.total > lo; ++capa) for (int capb = 1; capb <= 40 && best.total > lo; ++capb) for (const Ring &r : rings) {
        const int t = v6_layout(v6_rows_bytes(capa, capb, noll), (capa + 3) & ~3, r.r).total;
        if (t >= lo && t < best.total) { const Found f = {capa, capb, r.k0, r.k1, r.extra, t}; best = f; if (t == lo) break; }
    }
    if (best.total > hi) { fprintf(stderr, "no v6 plan of %d .. %d bytes\n", lo, hi); exit(3); }
    return best;
}
// at the limit and one step above it: 16 bytes, or the next size a plan can have (a Noll 3 plan's size / 16 is never 5 mod 6)
static void v6_limit(const char *what, int noll, int limit, const PrepOptions &o)
{
    for (int step = 0; step < 2; ++step) {
        const Found f = step ? find_v6(noll, limit + 16, limit + 48) : find_v6(noll, limit, limit);
        Tables ta(200, 2, 2, 3), tb(300, f.k0, f.k1, f.k1 + 1); tb.longer(1, 150, f.extra);
        const DpFacts d = dp(2, noll, ta, 200, tb, 300, f.capa, f.capb);
        char name[160];
        snprintf(name, sizeof name, "kind 2 Noll %d, %s: v6 plan of %d bytes (capa %d capb %d lists %d / %d + %d)", noll, what, f.total, f.capa, f.capb, f.k0, f.k1, f.extra);
        show(name, d, shape_base(), o);
    }
}
// an _hf DP whose v3 plan with LDS lists has exactly `total` bytes
static void v3_limit(int total, const PrepOptions &o, const char *what)
{
    Tables tb(300, 0, 0, 0);
    for (int capa = 1; capa <= 400; ++capa) for (int k = 1100; k <= 14000; ++k) {       // k entries in the s lists of the 64 rows, spread evenly (17 and more each)
        Tables ta(64, k / 64, 0, 0);
        for (int r = 0; r < k % 64; ++r) ta.longer(0, r, 1);
        DpFacts d = dp(1, 2, ta, 64, tb, 300, capa, 0);
        d.a.maxlist = k / 64 + 2;
        const int t = v3_need(d, 128).total;
        if (t > total) break;
        if (t != total) { k += (total - t) / 12 > 8 ? (total - t) / 12 - 8 : 0; continue; }
        char name[160];
        snprintf(name, sizeof name, "kind 1, v3 plan of %d bytes%s (capa %d, %d entries in 64 rows)", total, what, capa, k);
        show(name, d, shape_base(), o);
        d.a.len = 32768; snprintf(name, sizeof name, "kind 1, v3 plan of %d bytes%s, a side of 32768 columns", total, what); show(name, d, shape_base(), o);
        return;
    }
    fprintf(stderr, "no v3 plan of %d bytes\n", total); exit(3);
}
static void run_choose()
{
    const PrepOptions o0 = prep_defaults(256);
    const BatchShape s0 = shape_base();
    Tables ta(200, 2, 2, 3), tb(300, 2, 2, 3);
    {   // kind 0
        DpFacts d = dp(0, 2, ta, 200, tb, 300);
        show("kind 0", d, s0, o0);
        { DpFacts r = d; r.rect = 1; show("kind 0, rect", r, s0, o0); }
        { PrepOptions o = o0; o.force_v1 = true; show("kind 0, FORCE_V1", d, s0, o); }
        { PrepOptions o = o0; o.no_v7 = true; show("kind 0, NO_V7", d, s0, o); }
        show("kind 0, force_v1 argument", d, s0, o0, true);
    }
    {   // kind 3: every crg2_kind at its member limit and one beyond
        const int ck[7] = {11, 120, 121, 210, 211, 220, 221}, an[7] = {1, 1, 1, 5, 5, 3, 3}, bn[7] = {1, 5, 5, 1, 1, 3, 3}, da[7] = {1, 0, 0, 1, 1, 1, 1}, db[7] = {0, 1, 1, 0, 0, 0, 0};
        for (int c = 0; c < 7; ++c) for (int beyond = 0; beyond < 2; ++beyond) for (int wt = 0; wt < 2; ++wt) {
            DpFacts d = dp(3, 2 + (c & 1), ta, 200, tb, 300);
            d.crg2_kind = ck[c]; d.a.many = an[c] + beyond * da[c]; d.b.many = bn[c] + beyond * db[c];
            d.a.gapdens = d.b.gapdens = d.a.postgapdens = d.b.postgapdens = true; d.a.weight = d.b.weight = wt != 0;
            char name[96];
            snprintf(name, sizeof name, "kind 3, crg2 %d, %d x %d members, %s", ck[c], d.a.many, d.b.many, wt ? "weights" : "no weights");
            show(name, d, s0, o0);
        }
        DpFacts d = dp(3, 2, ta, 200, tb, 300);
        d.crg2_kind = 220; d.a.many = 3; d.b.many = 3; d.a.gapdens = d.b.gapdens = d.a.postgapdens = d.b.postgapdens = true;
        { DpFacts x = d; x.a.gapdens = false; show("kind 3, a without gapdens", x, s0, o0); }
        { DpFacts x = d; x.b.postgapdens = false; show("kind 3, b without postgapdens", x, s0, o0); }
        { DpFacts x = d; x.crg2_kind = 221; x.a.weight = true; show("kind 3, crg2 221, b without weights", x, s0, o0); }
        { DpFacts x = d; x.crg2_kind = 7; show("kind 3, an unknown crg2", x, s0, o0); }
        { PrepOptions o = o0; o.no_v8 = true; show("kind 3, NO_V8", d, s0, o); }
        { PrepOptions o = o0; o.force_v1 = true; show("kind 3, FORCE_V1", d, s0, o); }
        show("kind 3, force_v1 argument", d, s0, o0, true);
    }
    {   // kind 1
        DpFacts d = dp(1, 2, ta, 200, tb, 300);
        show("kind 1", d, s0, o0);
        { DpFacts x = d; x.a.maxlist = 16; show("kind 1, a.maxlist 16", x, s0, o0); x.a.maxlist = 17; show("kind 1, a.maxlist 17", x, s0, o0); }
        { DpFacts x = d; x.a.r_from_t = 0; show("kind 1, r_from_t 0", x, s0, o0); }
        { DpFacts x = d; x.a.len = 32499; x.b.len = 32500; show("kind 1, a.len + b.len 64999", x, s0, o0); x.b.len = 32501; show("kind 1, a.len + b.len 65000", x, s0, o0); }
        { DpFacts x = d; x.a.maxlist = 17; x.a.len = 32767; show("kind 1, lists in LDS, a side of 32767 columns", x, s0, o0); x.a.len = 32768; show("kind 1, lists in LDS, a side of 32768 columns", x, s0, o0); }
        { DpFacts x = d; x.a.maxlist = 17; x.a.len = 300; x.b.len = 32767; show("kind 1, lists in LDS, b side of 32767 columns", x, s0, o0); x.b.len = 32768; show("kind 1, lists in LDS, b side of 32768 columns", x, s0, o0); }
        { PrepOptions o = o0; o.no_areg = true; show("kind 1, NO_AREG", d, s0, o); }
        { PrepOptions o = o0; o.force_v2 = true; show("kind 1, FORCE_V2", d, s0, o); }
        { PrepOptions o = o0; o.force_v1 = true; show("kind 1, FORCE_V1", d, s0, o); }
        show("kind 1, force_v1 argument", d, s0, o0, true);
        const int third = (int) V2_LDS_MAX / 3 & ~15, whole = (int) V2_LDS_MAX;
        v3_limit(third, o0, ", just at a third of the LDS"); v3_limit(third + 16, o0, ", just above a third of the LDS");
        v3_limit(whole, o0, ", the whole LDS"); v3_limit(whole + 16, o0, ", above the LDS");
        { PrepOptions o = o0; o.no_areg = true; v3_limit(third + 16, o, ", just above a third of the LDS, NO_AREG"); }
        {   // v3r's own plan (lists in registers) at and above the LDS: capacity decides
            for (int capa = 1; capa <= 400; ++capa) {
                DpFacts x = dp(1, 2, ta, 200, tb, 300, capa, 0);
                const int t = v3_need(x, 128, true).total;
                if (t == whole || t == whole + 16 || (t > whole && v3_need(dp(1, 2, ta, 200, tb, 300, capa - 1, 0), 128, true).total < whole)) { char name[96]; snprintf(name, sizeof name, "kind 1, v3r plan of %d bytes (capa %d)", t, capa); show(name, x, s0, o0); x.capa = capa - 1; snprintf(name, sizeof name, "kind 1, v3r plan of %d bytes (capa %d)", v3_need(x, 128, true).total, capa - 1); show(name, x, s0, o0); break; }
            }
        }
    }
    {   // kind 2
        DpFacts d = dp(2, 2, ta, 200, tb, 300);
        show("kind 2, v6_on", d, s0, o0);
        { BatchShape s = s0; s.v6_on = false; show("kind 2, v6 off", d, s, o0); }
        { DpFacts x = d; x.a.maxlist = 16; show("kind 2, Noll 2, a.maxlist 16", x, s0, o0); x.a.maxlist = 17; show("kind 2, Noll 2, a.maxlist 17", x, s0, o0); }
        { DpFacts x = d; x.noll = 3; x.a.maxlist = 10; show("kind 2, Noll 3, a.maxlist 10", x, s0, o0); x.a.maxlist = 11; show("kind 2, Noll 3, a.maxlist 11", x, s0, o0); }
        { DpFacts x = d; x.a.r_from_t = 0; show("kind 2, a.r_from_t 0", x, s0, o0); }
        { DpFacts x = d; x.b.r_from_t = 0; show("kind 2, b.r_from_t 0", x, s0, o0); }
        { PrepOptions o = o0; o.no_v6 = true; show("kind 2, NO_V6", d, s0, o); }
        { PrepOptions o = o0; o.force_v2 = true; show("kind 2, FORCE_V2", d, s0, o); }
        { PrepOptions o = o0; o.force_v1 = true; show("kind 2, FORCE_V1", d, s0, o); }
        { DpFacts x = d; x.a.len = 32499; x.b.len = 32500; show("kind 2, a.len + b.len 64999", x, s0, o0); x.b.len = 32501; show("kind 2, a.len + b.len 65000", x, s0, o0); }
        v6_limit("default limit", 2, 40 * 1024, o0); v6_limit("default limit", 3, 40 * 1024, o0);
        { PrepOptions o = o0; o.v6_small = 53 * 1024; v6_limit("V6_SMALL_KB=53", 2, 53 * 1024, o); v6_limit("V6_SMALL_KB=53, at the class A limit", 2, 40 * 1024, o); }
        { PrepOptions o = o0; o.v6_large = 96 * 1024; v6_limit("V6_LARGE_KB=96", 2, 96 * 1024, o); v6_limit("V6_LARGE_KB=96, at the class A limit", 3, 40 * 1024, o); }
        { PrepOptions o = o0; o.v6_small = 53 * 1024; o.v6_large = 96 * 1024; v6_limit("V6_SMALL_KB=53 V6_LARGE_KB=96", 2, 53 * 1024, o); v6_limit("V6_SMALL_KB=53 V6_LARGE_KB=96", 2, 96 * 1024, o); }
        // v2's own limit: the longest lists that fit 160 KB and one entry more, with 256 and with 128 threads
        for (int T = 256; T >= 128; T -= 128) {
            BatchShape s = s0; s.v6_on = false; s.v2_threads = T;
            for (int noll = 2; noll <= 3; ++noll) {
                DpFacts x = dp(2, noll, ta, 200, tb, 300, 20, 20);
                int ml = 1;
                while (v2_lds_bytes(2, noll, 20, 20, ml + 1, ml + 1, T) + 4 * T <= V2_LDS_MAX) ++ml;
                for (int k = 0; k < 2; ++k) {
                    x.a.maxlist = x.b.maxlist = ml + k;
                    char name[128];
                    snprintf(name, sizeof name, "kind 2 Noll %d, v6 off, %d threads, lists of %d: %zu bytes on v2", noll, T, ml + k, v2_lds_bytes(2, noll, 20, 20, ml + k, ml + k, T) + 4 * T);
                    show(name, x, s, o0);
                }
            }
        }
    }
    {   // the intron-position bonus on top of every generation
        struct { const char *what; DpFacts d; PrepOptions o; } c[6] = {{"7", dp(0, 2, ta, 200, tb, 300), o0}, {"8", dp(3, 2, ta, 200, tb, 300), o0}, {"6", dp(2, 2, ta, 200, tb, 300), o0},
                                                                     {"3", dp(1, 2, ta, 200, tb, 300), o0}, {"2", dp(1, 2, ta, 200, tb, 300), o0}, {"1", dp(2, 2, ta, 200, tb, 300), o0}};
        c[1].d.crg2_kind = 11; c[1].d.a.many = c[1].d.b.many = 1; c[1].d.a.gapdens = c[1].d.b.gapdens = c[1].d.a.postgapdens = c[1].d.b.postgapdens = true;
        c[4].d.a.maxlist = 17; c[5].o.no_v6 = true;
        for (int k = 0; k < 6; ++k) {
            char name[128];
            DpFacts d = c[k].d;
            snprintf(name, sizeof name, "generation %s without a bonus table", c[k].what); show(name, d, s0, c[k].o);
            d.nbonus = 5;
            snprintf(name, sizeof name, "nbonus 5 on generation %s", c[k].what); show(name, d, s0, c[k].o);
            { BatchShape s = s0; s.v2_sweep = 0; snprintf(name, sizeof name, "nbonus 5 on generation %s, v2_sweep 0", c[k].what); show(name, d, s, c[k].o); }
            { PrepOptions o = c[k].o; o.no_strip_bonus = true; snprintf(name, sizeof name, "nbonus 5 on generation %s, NO_STRIP_BONUS", c[k].what); show(name, d, s0, o); }
            { DpFacts x = d; x.b.len = 32768; snprintf(name, sizeof name, "nbonus 5 on generation %s, b side of 32768 columns", c[k].what); show(name, x, s0, c[k].o); }
            { snprintf(name, sizeof name, "nbonus 5 on generation %s, force_v1 argument", c[k].what); show(name, d, s0, c[k].o, true); }
        }
        DpFacts r = dp(0, 2, ta, 200, tb, 300); r.rect = 1; r.nbonus = 5; show("nbonus 5 on a rect DP (generation 0)", r, s0, o0);
    }
}

static void show(const char *name, const std::vector<DpFacts> &f, const PrepOptions &o)
{
    const BatchShape s = batch_shape(f.data(), (int) f.size(), o);
    printf("%s: v3_cols %d v2_threads %d v2_cols %d v6_on %d v3_sweep %d v2_sweep %d\n", name, s.v3_cols, s.v2_threads, s.v2_cols, s.v6_on ? 1 : 0, s.v3_sweep, s.v2_sweep);
}
static void run_shape()
{
    const PrepOptions o0 = prep_defaults(256);
    Tables t(4200, 0, 0, 0);
    char name[128];
    show("n = 0", std::vector<DpFacts>(), o0);
    // pick(1, 64, 128, 32, 4 ncu): one _hf DP of S 64-row strips and many columns offers S tiles at a time; 4 S >= 5 x 1024 from 1280
    for (int S = 1279; S <= 1280; ++S) {
        std::vector<DpFacts> f;
        for (int k = 0; k < S / 64; ++k) f.push_back(dp(1, 2, t, 64 * 64, t, 64 * 128));
        if (S % 64) f.push_back(dp(1, 2, t, 64 * (S % 64), t, 64 * 128));
        snprintf(name, sizeof name, "_hf: %d tiles of 128 columns at a time", S); show(name, f, o0);
    }
    {   // ... and at 64 / 32 columns: DPs of 128 columns have 1 / 2 / 4 blocks
        std::vector<DpFacts> f;
        for (int k = 0; k < 640; ++k) f.push_back(dp(1, 2, t, 4096, t, 128));
        show("_hf: 640 DPs of 128 columns (1280 tiles at 64 columns)", f, o0);
        f.pop_back(); show("_hf: 639 DPs of 128 columns (1278 tiles at 64 columns, 2556 at 32)", f, o0);
        f.resize(319); show("_hf: 319 DPs of 128 columns (1276 tiles at 32 columns)", f, o0);
    }
    // pick(2, 16, 128, 64, 6 ncu): v2_threads; then pick(2, R, 512, 64, ncu x 768 / threads): v2_cols
    for (int S = 1919; S <= 1920; ++S) {
        std::vector<DpFacts> f;
        for (int k = 0; k < S / 64; ++k) f.push_back(dp(2, 2, t, 16 * 64, t, 128 * 64));
        if (S % 64) f.push_back(dp(2, 2, t, 16 * (S % 64), t, 128 * 64));
        snprintf(name, sizeof name, "_pf: %d tiles of 16 rows x 128 columns at a time", S); show(name, f, o0);
        PrepOptions o = o0;
        o.v2_threads = 128; snprintf(name, sizeof name, "_pf: %d tiles, V2_THREADS=128", S); show(name, f, o);
        o.v2_threads = 256; snprintf(name, sizeof name, "_pf: %d tiles, V2_THREADS=256", S); show(name, f, o);
        o.v2_threads = 192; snprintf(name, sizeof name, "_pf: %d tiles, V2_THREADS=192 (ignored)", S); show(name, f, o);
    }
    for (int T = 128; T <= 256; T += 128) {       // v2_cols: 4 par >= 5 ncu x 768 / T, DPs of 512 columns (1 block at 512, 2 at 256, ...)
        const int slots = 256 * (768 / T), thr = (5 * slots + 3) / 4;
        for (int S = thr - 1; S <= thr; ++S) {
            std::vector<DpFacts> f;
            for (int k = 0; k < S; ++k) f.push_back(dp(2, 2, t, 4096, t, 512));
            PrepOptions o = o0; o.v2_threads = T;
            snprintf(name, sizeof name, "_pf, %d threads: %d DPs of 512 columns", T, S); show(name, f, o);
            f.resize((S + 1) / 2); snprintf(name, sizeof name, "_pf, %d threads: %d DPs of 512 columns", T, (S + 1) / 2); show(name, f, o);
        }
    }
    {
        std::vector<DpFacts> f(1, dp(2, 2, t, 640, t, 900));
        f.push_back(dp(1, 2, t, 640, t, 900));
        const int cols[4] = {15, 16, 4096, 4097};
        for (int k = 0; k < 4; ++k) {
            PrepOptions o = o0;
            o.v2_cols = cols[k]; snprintf(name, sizeof name, "V2_COLS=%d", cols[k]); show(name, f, o);
            o = o0; o.v3_cols = cols[k]; snprintf(name, sizeof name, "V3_COLS=%d", cols[k]); show(name, f, o);
        }
        { PrepOptions o = o0; o.v3_sweep = 0; show("V3_SWEEP=0", f, o); }
        { PrepOptions o = o0; o.v2_sweep = 0; show("V2_SWEEP=0", f, o); o.v2_sweep = 16; show("V2_SWEEP=16", f, o); }
        { PrepOptions o = o0; o.min_strips_set = true; o.min_strips = 0; show("V6_MIN_STRIPS=0", f, o); show("V6_MIN_STRIPS=0, n = 0", std::vector<DpFacts>(), o); }
        { PrepOptions o = o0; o.min_strips_set = true; o.min_strips = 10; show("V6_MIN_STRIPS=10, 10 strips", f, o); o.min_strips = 11; show("V6_MIN_STRIPS=11, 10 strips", f, o); }
    }
    for (int ncu = 8; ncu <= 256; ncu += 248) for (int S = 35 * ncu - 1; S <= 35 * ncu; ++S) {       // s6 against 35 strips of 64 rows per CU
        std::vector<DpFacts> f;
        for (int k = 0; k < S / 64; ++k) f.push_back(dp(2, 2, t, 4096 - 63, t, 300));
        if (S % 64) f.push_back(dp(2, 2, t, 64 * (S % 64), t, 300));
        f.push_back(dp(1, 2, t, 4096, t, 300));                          // (an _hf DP does not count)
        snprintf(name, sizeof name, "%d CUs, %d _pf strips of 64 rows", ncu, S); show(name, f, prep_defaults(ncu));
    }
}

struct QCase {
    std::vector<DpFacts> f; std::vector<KernelChoice> c; std::vector<long long> cells;
    void add(const DpFacts &d, int gen, int ib = 0) { const KernelChoice k = {gen, (char) ib, 0, {{32, 32, V6_RHCOLS}, 4, {1, 1, 1}}}; f.push_back(d); c.push_back(k); cells.push_back(d.kind < 0 ? 0 : (long long) (d.a.right - d.a.left) * (d.b.right - d.b.left) - 7); }
    void chosen(const DpFacts &d, const BatchShape &s, const PrepOptions &o) { const KernelChoice k = choose_kernel(d, s, o, false); if (k.generation != 6) { fprintf(stderr, "a queue case wanted a v6 DP\n"); exit(3); } add(d, 6); c.back() = k; }
};
static void show(const char *name, const QCase &q, const BatchShape &s, const PrepOptions &o)
{
    const int n = (int) q.f.size();
    const QueuePlan Q = queue_plan(q.f.data(), q.c.data(), q.cells.data(), s, o, n);
    printf("%s: %d DPs, %zu tiles%s\n", name, n, Q.tiles.size(), Q.bad >= 0 ? ", refused: a DP without a variant slot" : "");
    if (Q.bad >= 0) return;
    for (size_t k = 0; k < Q.tiles.size(); ++k) { const V2Tile &T = Q.tiles[k]; printf("  tile %zu: prob %d ti %d tj %d nsteps %d self %d up %d left %d diag %d war %d\n", k, T.prob, T.ti, T.tj, T.nsteps, T.self, T.dep_up, T.dep_left, T.dep_diag, T.dep_war); }
    printf("  var_off:"); for (int v = 0; v <= G2G_NVAR; ++v) printf(" %d", Q.var_off[v]); printf("\n");
    printf("  var_cells:"); for (int v = 0; v < G2G_NVAR; ++v) if (Q.var_cells[v]) printf(" %d:%lld", v, Q.var_cells[v]); printf("\n");
    printf("  flags:");
    for (size_t k = 0; k < Q.flags.size(); ) { size_t e = k; while (e < Q.flags.size() && Q.flags[e] == Q.flags[k]) ++e; printf(" %d x %zu", Q.flags[k], e - k); k = e; }
    printf("\n  fail_off %d dump_off %d xq_off %d nflags %zu\n", Q.fail_off, Q.dump_off, Q.xq_off, Q.flags.size());
    printf("  ip:"); for (size_t k = 0; k < Q.ip.size(); ++k) printf(" %d", Q.ip[k]); printf("\n");
    printf("  lds2p %zu v2_maxrows %d v2_maxcols %d simtile_lds %zu\n", Q.lds2p, Q.v2_maxrows, Q.v2_maxcols, Q.simtile_lds);
    for (int sl = 0; sl < G2G_NVAR; ++sl) {
        if (Q.var_off[sl + 1] == Q.var_off[sl]) continue;
        if (variant_v3_index(sl) >= 0) { const V3Lds &L = Q.v3lds[variant_v3_index(sl)]; printf("  v3lds[%d]: rows %d black %d stsc %d aglen %d afreq %d boff %d bglen %d bfreq %d svals %d sink %d total %d\n", variant_v3_index(sl), L.rows, L.black, L.stsc, L.aglen, L.afreq, L.boff, L.bglen, L.bfreq, L.svals, L.sink, L.total); }
        if (variant_v6_index(sl) >= 0) { const V6Lds &L = Q.v6lds[variant_v6_index(sl)]; printf("  v6lds[%d]: rows %d black %d stsc %d svals %d sink %d total %d ringk %d %d %d ringf %d %d %d rs %d %d %d rtail %d\n", variant_v6_index(sl), L.rows, L.black, L.stsc, L.svals, L.sink, L.total, L.ringk[0], L.ringk[1], L.ringk[2], L.ringf[0], L.ringf[1], L.ringf[2], L.rs[0], L.rs[1], L.rs[2], L.rtail); }
    }
    printf("  V6_RING_PLAN \"%s\"\n", Q.v6_ring_plan.c_str());
}
static void run_queues()
{
    const PrepOptions o0 = prep_defaults(256);
    const BatchShape s0 = shape_base();
    Tables t(700, 2, 2, 3);
    char name[128];
    show("n = 0", QCase(), s0, o0);
    // DPs of 1, R and R + 1 rows: R = 16 and 32 on v2 (128 / 256 threads), R = 64 on v3r, v6, v7, v8
    for (int T = 128; T <= 256; T += 128) {
        BatchShape s = s0; s.v2_threads = T;
        const int R = T / 8, rows[3] = {1, R, R + 1};
        QCase q;
        for (int k = 0; k < 3; ++k) q.add(dp(k == 1 ? 1 : 2, 2 + (k & 1), t, rows[k], t, 90), 1);
        snprintf(name, sizeof name, "v2, %d threads: DPs of 1, %d and %d rows", T, R, R + 1); show(name, q, s, o0);
    }
    {
        PrepOptions o = o0; o.min_strips_set = true; o.min_strips = 0;
        const int rows[3] = {1, 64, 65};
        QCase q;
        for (int k = 0; k < 3; ++k) { q.add(dp(1, 2, t, rows[k], t, 90), 3); q.chosen(dp(2, 2, t, rows[k], t, 90), s0, o); q.add(dp(0, 2, t, rows[k], t, 90), 7); q.add(dp(3, 3, t, rows[k], t, 90, 3, 3), 8); }
        show("v3r, v6, v7, v8: DPs of 1, 64 and 65 rows", q, s0, o);
    }
    {   // a band so narrow that the lower strips hold no cell
        QCase q;
        DpFacts d = dp(1, 2, t, 200, t, 20); d.lw = -3; d.up = 2; q.add(d, 3);
        DpFacts e = dp(2, 2, t, 70, t, 20); e.lw = -3; e.up = 2; q.add(e, 1);
        show("narrow bands: strips without a cell", q, s0, o0);
        BatchShape s = s0; s.v2_sweep = 0; s.v3_sweep = 0; s.v2_cols = 16; s.v3_cols = 16;
        show("narrow bands, tile mode: tiles without a cell", q, s, o0);
    }
    {   // tile mode with three and more column blocks
        BatchShape s = s0; s.v2_sweep = 0; s.v3_sweep = 0; s.v2_cols = 64; s.v3_cols = 32;
        QCase q;
        q.add(dp(2, 2, t, 100, t, 200), 1); q.add(dp(1, 2, t, 200, t, 100), 3); q.add(dp(1, 3, t, 130, t, 97), 2); q.add(dp(1, 2, t, 100, t, 200), 1);
        DpFacts band = dp(1, 2, t, 200, t, 220); band.lw = -10; band.up = 30; q.add(band, 3);
        show("tile mode: v2 with 64-column tiles, v3 / v3r with 32-column tiles", q, s, o0);
        show("sweep mode, the same DPs", q, s0, o0);
        PrepOptions o = o0; o.no_chainq = true;
        show("sweep mode, NO_CHAINQ", q, s0, o);
        q.add(dp(0, 2, t, 70, t, 90), 7); q.add(dp(3, 2, t, 70, t, 90, 3, 3), 8);
        show("NO_CHAINQ with v7 and v8 DPs: their chains stay queue entries", q, s0, o);
        BatchShape s2 = s0; s2.v3_sweep = 0;
        show("v3 in tile mode, v2 in sweep mode", q, s2, o0);
    }
    {   // an invalid DP between valid ones, and one on g2g_forward_kernel
        QCase q;
        DpFacts bad = dp(1, 2, t, 10, t, 10); bad.kind = -1;
        q.add(dp(1, 2, t, 70, t, 90), 3); q.add(bad, 0); q.add(dp(2, 2, t, 70, t, 90), 0); q.add(dp(0, 3, t, 70, t, 90), 7);
        show("an invalid DP and a v1 DP between valid ones", q, s0, o0);
        PrepOptions o = o0; o.inject = true;
        o.inject_victim = 3; show("INJECT_STALL=3 (a DP with strips)", q, s0, o);
        o.inject_victim = 2; show("INJECT_STALL=2 (a DP without strips)", q, s0, o);
        o.inject_victim = 0; show("INJECT_STALL=0", q, s0, o);
    }
    {   // the column-score tiles' LDS
        QCase q;
        DpFacts d = dp(1, 2, t, 70, t, 90); d.sim2_kind = 31; d.a.nelm = 21; d.a.felm = 0; d.b.many = 7; q.add(d, 3);
        show("sim31: profile rows of a, residues of b", q, s0, o0);
        DpFacts e = dp(2, 2, t, 70, t, 90); e.sim2_kind = 330; e.a.nelm = 25; e.a.felm = 4; e.b.nelm = 25; e.b.felm = 4; q.add(e, 1);
        show("... and sim33_n: frequency vectors of b", q, s0, o0);
        DpFacts g = dp(1, 2, t, 70, t, 90); g.sim2_kind = 33; g.a.nelm = 0; QCase q2; q2.add(g, 3);
        show("sim33 without profile rows", q2, s0, o0);
    }
    {   // one batch that fills slots of every family, _ib slots included; v6 of classes A, B and C
        PrepOptions o = o0; o.min_strips_set = true; o.min_strips = 0; o.v6_small = 53 * 1024; o.v6_large = 96 * 1024;
        QCase q;
        std::vector<Tables *> keep;                   // b's tables of the v6 DPs (they live as long as the cases)
        for (int noll = 2; noll <= 3; ++noll) {
            q.add(dp(1, noll, t, 70, t, 90), 1); q.add(dp(2, noll, t, 70, t, 90), 1); q.add(dp(1, noll, t, 70, t, 90, 9), 2); q.add(dp(1, noll, t, 130, t, 90), 3);
            q.add(dp(0, noll, t, 70, t, 90), 7); q.add(dp(3, noll, t, 70, t, 90, 3, 3), 8);
            q.add(dp(0, noll, t, 70, t, 90), 7, 1); q.add(dp(1, noll, t, 70, t, 90), 1, 1); q.add(dp(2, noll, t, 70, t, 90, 6, 5), 1, 1); q.add(dp(3, noll, t, 70, t, 90, 2, 2), 8, 1);
            const int target[3] = {36 * 1024, 48 * 1024, 80 * 1024};
            for (int cls = 0; cls < 3; ++cls) for (int step = 0; step < 2; ++step) {
                const Found f = find_v6(noll, target[cls] + 1024 * step, target[cls] + 1024 * step + 512);
                Tables *tb = new Tables(300, f.k0, f.k1, f.k1 + 1); tb->longer(1, 150, f.extra);
                q.chosen(dp(2, noll, t, 130 + 64 * step, *tb, 300, f.capa, f.capb), s0, o);
                keep.push_back(tb);
            }
        }
        show("every family, _ib slots, v6 classes A, B and C", q, s0, o);
        PrepOptions o1 = o; o1.v6_small = 40 * 1024;
        QCase q1;
        for (size_t k = 0; k < q.f.size(); ++k) if (q.c[k].generation == 6 && q.c[k].v6_total <= o1.v6_large) q1.chosen(q.f[k], s0, o1);
        show("the v6 DPs with V6_LARGE_KB=96 alone: classes A and C", q1, s0, o1);
        QCase bad; bad.add(dp(1, 2, t, 70, t, 90), 3, 1);
        show("a bonus table on v3r: no such slot", bad, s0, o0);
        for (size_t k = 0; k < keep.size(); ++k) delete keep[k];
        keep.clear();
    }
}

int main(int argc, char **argv)
{
    const char *what = argc > 1 ? argv[1] : "";
    if (!strcmp(what, "slots")) run_slots();
    else if (!strcmp(what, "shares")) run_shares();
    else if (!strcmp(what, "launches")) run_launches();
    else if (!strcmp(what, "report")) run_report();
    else if (!strcmp(what, "choose")) run_choose();
    else if (!strcmp(what, "shape")) run_shape();
    else if (!strcmp(what, "queues")) run_queues();
    else { fprintf(stderr, "usage: plan_main slots | shares | launches | report | choose | shape | queues\n"); return 2; }
    return 0;
}
