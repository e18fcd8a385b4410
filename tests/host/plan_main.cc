// plan_main.cc -- runs the host-side planning of prrn_aln_amd/csrc/g2g_plan.h over a fixed list of cases and prints one line
// per result (tests/test_host_plan.py compares the output with tests/golden/host_plan/*.txt).  No GPU, no HIP.
//   plan_main slots | shares | launches | report
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

int main(int argc, char **argv)
{
    const char *what = argc > 1 ? argv[1] : "";
    if (!strcmp(what, "slots")) run_slots();
    else if (!strcmp(what, "shares")) run_shares();
    else if (!strcmp(what, "launches")) run_launches();
    else if (!strcmp(what, "report")) run_report();
    else { fprintf(stderr, "usage: plan_main slots | shares | launches | report\n"); return 2; }
    return 0;
}
