// g2g_lds.h -- LDS geometry that the one-lane-per-cell strip kernels and the host's plans (g2g_plan.h) must agree on: the pitch
// of a row of dynamic lists, the inline part of a list, and the plan and window constants of the v6 launches.  Plain C++ (it
// compiles with g++ for tests/host/*.cc); the kernels include it for the same definitions.
#ifndef G2G_LDS_H
#define G2G_LDS_H

#ifndef G2G_HD
#if defined(__HIPCC__)
#define G2G_HD __host__ __device__
#else
#define G2G_HD
#endif
#endif

G2G_HD inline int v3_pitch(int nslot, int lsz)            // dwords per LDS row: odd number of 16-B units
{
    int p = nslot * lsz;
    if (((p >> 2) & 1) == 0) p += 4;
    return p;
}

// dwords of a dynamic list that a v6 strip keeps in LDS (its INLINE part; see LS6 in g2g_kernels_v6.hip)
G2G_HD inline int v6_inline_dw(int cap4) { return cap4 <= 4 ? 4 : cap4 <= 16 ? 8 : cap4 <= 32 ? 16 : cap4 <= 64 ? 32 : cap4; }

// LDS plan of a v6 launch, byte offsets.  Per view (s, t) the column-list ring has rs[v] entries (a multiple of 32, any) followed
// by a MIRRORED TAIL of rtail entries: freq at ringf[v] (f64), lookup keys at ringk[v] (u32).  View 2 (r) has no ring of its own:
// ringf[2] is an array of V6_RHCOLS head freqs, one per column.
struct V6Lds { int rows, black, stsc, svals, sink, total; int ringk[3], ringf[3], rs[3], rtail; };

// The ring's feed schedule.  A strip refills every V6_FEED steps, at a step where lane 0 stands on column n0, up to column
// n0 + V6_AHEAD.  Until the next refill lane 0 moves on to n0 + V6_FEED - 1, and a lane reads the ring only for the column it
// stands on (the one-step-ahead register pipelines read the offset tables in HBM, not the ring): the furthest column read before
// the next refill is n0 + V6_FEED - 1 = n0 + 15, five columns inside the read-ahead.  The lowest live column at a refill is lane
// 63's, n0 - 63; so 64 + V6_AHEAD columns must fit a ring together, and V6_WINDOW keeps four more.
#define V6_FEED 16                      // columns per ring refill
#define V6_AHEAD 20                     // a refill reaches this many columns beyond lane 0's (>= V6_FEED - 1)
#define V6_WINDOW (64 + V6_AHEAD + 4)   // columns whose lists must fit the ring together
#define V6_RHCOLS 128                   // columns of the per-column array of r-list heads (a power of 2 >= V6_WINDOW)
static_assert(V6_AHEAD >= V6_FEED - 1 && V6_RHCOLS >= V6_WINDOW && (V6_RHCOLS & (V6_RHCOLS - 1)) == 0, "v6 ring windows");

// byte offsets of the LDS regions of a v3 launch (host: v3_layout of g2g_plan.h)
struct V3Lds { int rows, black, stsc, aglen, afreq, boff, bglen, bfreq, svals, sink, total; };

// A queue entry of a persistent kernel: tile (ti, tj) of DP prob (ti -1 / -2: its top / left boundary chain), nsteps steps;
// self / dep_*: indices into the batch's tile-completion flags (-1: no such neighbour)
struct V2Tile { int prob, ti, tj, nsteps, self, dep_up, dep_left, dep_diag, dep_war; };

// Longest static list (terminator included) a kernel keeps in registers: what the host's kernel choice tests
#ifndef G2G_V3_NA
#define G2G_V3_NA 16                    // v3r
#endif
#ifndef G2G_V6_NA
#define G2G_V6_NA 16
#endif
#ifndef G2G_V6_NA3
#define G2G_V6_NA3 10                   /* Noll 3: two more records per cell -- with 16-entry row lists the kernel would spill 94 registers */
#endif
#define V8_REC 12                       // v8: dwords of a record in HBM / in the staging slots

// the tiled column-score kernel (g2g_v2_sim_tile_kernel): rows x columns of a block, and the scorers it knows
#define SIM_TR 64
#define SIM_TC 128
G2G_HD inline bool sim_tiled_kind(int k) { return k == 31 || k == 320 || k == 321 || k == 33 || k == 330; }

// d_flags (g2g_strip.h says what lives where and why)
#define G2G_FSTRIDE 64                  // ints between two tile flags / progress words
#define G2G_DUMP_STRIPS 580             // strips of one DP the first time-out dumps for the host ...
#define G2G_DUMP_WORDS 11               // ... words each: progress word, HW_ID, three markers, two publish columns, (step, place) of two waves
#define G2G_HDRN 104                    // header words: 4 + the snapshot (want, seen, offset of the polled word, the words at and below it; [48, 64): per-wave heartbeats); G2G_HDR + G2G_HDRN is a multiple of G2G_FSTRIDE, so every progress line IS one 128-byte line

#endif
