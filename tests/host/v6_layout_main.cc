// v6_layout_main.cc -- checks the LDS plan of the v6 launches (prrn_aln_amd/csrc/g2g_plan.h: v6_ring_need, v6_layout) on
// synthetic offset tables and on the recorded facts of the bench sweep's 16 large-ring divisions.  No GPU, no HIP.
//   v6_layout_main need | layout | bench16
// Prints one line per case and "FAIL ..." lines (exit status 1) for what does not hold; tests/test_host_v6_layout.py runs it.
#include <string.h>
#include "g2g_plan.h"

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { ++g_fail; printf("FAIL %s:%d (%s) ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } while (0)

// ---- a side's three offset tables from per-column list lengths (entries, terminators not counted) --------------------
struct Side {
    int len;
    std::vector<int32_t> off[3];
    std::vector<int> ll[3];         // [view][column + 1]: position -1 first, as in the pool
    const int32_t *p[3];
};
static void side_set(Side &s, const std::vector<int> &ls, const std::vector<int> &lt, const std::vector<int> &head)
{
    s.len = (int) ls.size();
    for (int v = 0; v < 3; ++v) {
        s.ll[v].assign(s.len + 1, 0);
        for (int c = 0; c < s.len; ++c) s.ll[v][c + 1] = v == 0 ? ls[c] : v == 1 ? lt[c] : lt[c] + (head[c] ? 1 : 0);      // r = [head] + t
        s.off[v].assign(s.len + 2, 0);
        for (int q = 0; q <= s.len; ++q) s.off[v][q + 1] = s.off[v][q] + s.ll[v][q] + 1;      // every position ends with a terminator
        s.p[v] = s.off[v].data();
    }
}
static unsigned g_rng = 12345;
static int rnd(int n) { g_rng = g_rng * 1664525u + 1013904223u; return (int) ((g_rng >> 8) % (unsigned) n); }

struct Named { const char *name; Side s; };
static std::vector<Named> sides()
{
    std::vector<Named> all;
    auto add = [&](const char *name, int len, int (*fs)(int, int), int (*ft)(int, int)) {
        std::vector<int> ls(len), lt(len), hd(len);
        for (int c = 0; c < len; ++c) { ls[c] = fs(c, len); lt[c] = ft(c, len); hd[c] = rnd(2); }
        all.push_back(Named());
        all.back().name = name;
        side_set(all.back().s, ls, lt, hd);
    };
    add("dense", 400, [](int, int) { return 5 + rnd(9); }, [](int, int) { return 4 + rnd(10); });
    add("sparse", 400, [](int, int) { return rnd(12) == 0 ? 1 + rnd(3) : 0; }, [](int, int) { return rnd(9) == 0 ? 1 : 0; });
    add("one huge list", 300, [](int c, int) { return c == 137 ? 15 : rnd(3); }, [](int c, int) { return c == 136 ? 14 : rnd(2); });
    add("lists only at the right edge", 350, [](int c, int len) { return c >= len - 6 ? 9 + rnd(4) : 0; }, [](int c, int len) { return c >= len - 5 ? 8 + rnd(4) : 0; });
    add("longest list in the last column", 200, [](int c, int len) { return c == len - 1 ? 13 : rnd(5); }, [](int c, int len) { return c == len - 1 ? 12 : rnd(5); });
    add("b shorter than the window", 70, [](int, int) { return 2 + rnd(7); }, [](int, int) { return 1 + rnd(8); });
    add("empty lists", 150, [](int, int) { return 0; }, [](int, int) { return 0; });
    for (Named &x : all) for (int v = 0; v < 3; ++v) x.s.p[v] = x.s.off[v].data();
    return all;
}

// ---- v6_ring_need against brute force --------------------------------------------------------------------------------
static void run_need()
{
    std::vector<Named> all = sides();
    for (Named &x : all) {
        const Side &s = x.s;
        const int ranges[][2] = {{0, s.len}, {3, s.len - 2}, {s.len / 3, s.len / 3 + 40}, {s.len - 1, s.len}};
        for (const auto &rg : ranges) {
            const int left = rg[0], right = rg[1];
            const V6Ring R = v6_ring_need(s.p, left, right);
            int longest = 0;
            for (int v = 0; v < 3; ++v) {
                // (1) the window rule, entry by entry: the most entries any V6_WINDOW consecutive columns of [left, right) hold
                int window = 1;
                for (int c = left; c < right; ++c) {
                    int sum = 0;
                    for (int q = c; q < c + V6_WINDOW && q < right; ++q) sum += s.ll[v][q + 1];
                    window = std::max(window, sum);
                    longest = std::max(longest, s.ll[v][c + 1]);
                }
                // (2) the feed schedule: a strip whose lane 0 starts at column cb refills at n0 = cb, cb + V6_FEED, ... up to column
                // min(n0 + V6_AHEAD, right - 1); lane 63 then stands on n0 - 63 (no lane reads left of cb): the live columns
                int live = 0;
                for (int cb = left; cb < right; ++cb)
                    for (int n0 = cb; n0 - 63 < right; n0 += V6_FEED) {
                        int sum = 0;
                        for (int q = std::max(n0 - 63, cb); q <= std::min(n0 + V6_AHEAD, right - 1); ++q) sum += s.ll[v][q + 1];
                        live = std::max(live, sum);
                    }
                CHECK(R.need[v] == window, "%s [%d, %d) view %d: need %d, brute force %d", x.name, left, right, v, R.need[v], window);
                CHECK(live <= R.need[v], "%s [%d, %d) view %d: the schedule keeps %d entries alive, need %d", x.name, left, right, v, live, R.need[v]);
                if (v < 2) {
                    CHECK(R.rs[v] % 32 == 0 && R.rs[v] >= 32 && R.rs[v] >= R.need[v] && R.rs[v] - R.need[v] < 32 + (R.need[v] < 32 ? 32 : 0),
                          "%s [%d, %d) view %d: ring %d for a need of %d", x.name, left, right, v, R.rs[v], R.need[v]);
                } else CHECK(R.rs[v] == V6_RHCOLS, "%s: r view %d", x.name, R.rs[v]);
            }
            CHECK(R.tail % 4 == 0 && R.tail > longest && R.tail <= longest + 4, "%s [%d, %d): tail %d, longest list %d", x.name, left, right, R.tail, longest);
            printf("%s [%d, %d): need %d %d rings %d %d tail %d\n", x.name, left, right, R.need[0], R.need[1], R.rs[0], R.rs[1], R.tail);
        }
    }
}

// ---- v6_layout: aligned, disjoint regions that end at `total` --------------------------------------------------------
static void check_layout(const char *name, int rows_bytes, int ca4, const V6Ring &R)
{
    const V6Lds L = v6_layout(rows_bytes, ca4, R);
    struct Reg { const char *what; int at, bytes; };
    const Reg reg[] = {
        {"rows", L.rows, rows_bytes}, {"black", L.black, 4 * (ca4 + 8)}, {"stsc", L.stsc, 4 * 28},
        {"s freq", L.ringf[0], 8 * (R.rs[0] + R.tail)}, {"t freq", L.ringf[1], 8 * (R.rs[1] + R.tail)}, {"r heads", L.ringf[2], 8 * V6_RHCOLS},
        {"s keys", L.ringk[0], 4 * (R.rs[0] + R.tail)}, {"t keys", L.ringk[1], 4 * (R.rs[1] + R.tail)},
        {"svals", L.svals, 4 * 64}, {"sink", L.sink, 4 * 64 + 16 * 64},
    };
    const int n = (int) (sizeof reg / sizeof reg[0]);
    int end = 0;
    for (int i = 0; i < n; ++i) {
        CHECK(reg[i].at % 16 == 0 && reg[i].at >= 0, "%s: %s at %d", name, reg[i].what, reg[i].at);
        for (int j = 0; j < i; ++j)
            CHECK(reg[i].at >= reg[j].at + reg[j].bytes || reg[j].at >= reg[i].at + reg[i].bytes, "%s: %s and %s overlap", name, reg[i].what, reg[j].what);
        end = std::max(end, reg[i].at + reg[i].bytes);
    }
    CHECK(L.total == ((end + 15) & ~15), "%s: total %d, regions end at %d", name, L.total, end);
    CHECK(L.rs[0] == R.rs[0] && L.rs[1] == R.rs[1] && L.rtail == R.tail, "%s: the plan carries %d %d %d", name, L.rs[0], L.rs[1], L.rtail);
    printf("%s: total %d\n", name, L.total);
}
static void run_layout()
{
    std::vector<Named> all = sides();
    for (Named &x : all) {
        const V6Ring R = v6_ring_need(x.s.p, 0, x.s.len);
        check_layout(x.name, v6_rows_bytes(7, 9, 2), 8, R);
        check_layout(x.name, v6_rows_bytes(21, 3, 3), 24, R);
    }
    const V6Ring odd = {{224, 736, V6_RHCOLS}, 12, {213, 725, 1}};
    check_layout("odd sizes", 26032 + 4, 10, odd);
}

// ---- the 16 balanced divisions of the bench sweep (256 proteins x 1024 aa, seed 1) -----------------------------------
// Recorded from the host builders: division, ca4 = capa rounded up to 4, the s and t need over a window of 88 columns, the
// longest list.  rows_bytes is 26 032 for all of them (six slots of 8 + 8 inline dwords).  With power-of-two rings and a window
// of 100 columns their plans took 44 128 - 44 160 B; each must now pass the class A test by itself, and so must the plan of a
// launch that holds all of them beside the rest of the sweep (largest s need there: 192 entries as well).
static void run_bench16()
{
    static const int F[16][5] = {
        {2, 16, 165, 470, 11}, {3, 16, 165, 470, 11}, {4, 8, 181, 725, 14}, {79, 12, 173, 556, 12}, {80, 12, 187, 666, 13}, {100, 12, 188, 666, 13},
        {101, 8, 186, 705, 13}, {164, 8, 191, 720, 14}, {219, 8, 181, 706, 13}, {243, 8, 182, 706, 13}, {244, 8, 183, 708, 13}, {305, 8, 184, 692, 13},
        {309, 8, 185, 692, 13}, {313, 8, 185, 692, 13}, {432, 8, 178, 705, 13}, {448, 8, 182, 709, 13},
    };
    CHECK(v6_rows_bytes(8, 8, 2) == 26032, "rows_bytes %d", v6_rows_bytes(8, 8, 2));
    V6Ring all = {{32, 32, V6_RHCOLS}, 4, {1, 1, 1}};
    int ca4max = 0;
    for (const auto &f : F) {
        V6Ring R;                   // what v6_ring_need returns for these needs
        for (int v = 0; v < 2; ++v) { R.need[v] = f[2 + v]; R.rs[v] = std::max(32, (f[2 + v] + 31) & ~31); }
        R.need[2] = 1; R.rs[2] = V6_RHCOLS;
        R.tail = (f[4] + 1 + 3) & ~3;
        const V6Lds L = v6_layout(26032, f[1], R);
        CHECK(L.total <= V6_CLASS_A && V6_CLASS_A == 40960, "division %d: %d B", f[0], L.total);
        CHECK(clamp_wpc((size_t) L.total, 4) == 4, "division %d: %d strips per CU", f[0], clamp_wpc((size_t) L.total, 4));
        printf("division %d: rings %d %d tail %d total %d\n", f[0], R.rs[0], R.rs[1], R.tail, L.total);
        v6_ring_max(all, R);
        ca4max = std::max(ca4max, f[1]);
    }
    const V6Lds L = v6_layout(26032, ca4max, all);
    CHECK(L.total <= V6_CLASS_A && clamp_wpc((size_t) L.total, 4) == 4, "the launch: %d B", L.total);
    printf("launch: rings %d %d tail %d total %d\n", all.rs[0], all.rs[1], all.tail, L.total);
}

int main(int argc, char **argv)
{
    const char *what = argc > 1 ? argv[1] : "";
    if (!strcmp(what, "need")) run_need();
    else if (!strcmp(what, "layout")) run_layout();
    else if (!strcmp(what, "bench16")) run_bench16();
    else { fprintf(stderr, "usage: v6_layout_main need | layout | bench16\n"); return 2; }
    return g_fail ? 1 : 0;
}
