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

#endif
