// g2g_strip.h -- what every strip kernel (g2g_kernels_v2 ... v8.hip) shares.  Included behind g2g_kernels.hip (sim2, NEVSEL,
// thk_at) and in front of the strip kernel files.  Two parts:
//
//  1. PRIMITIVES: bounded waits on progress words (g2g_wait_ge), publish (G2G_POST, chain_publish), the per-DP fail flag, the
//     fence / cross-strip access macros, team_sync, the wave-uniform descriptor copy (uni_prob), strip-local column scores
//     (SimBlk), record scalars and their DPP hand-down (RS, rs_up), the ring slot indices (SLOT_*).
//  2. THE SCAFFOLD of the one-lane-per-cell strips (v3_tile, v6_strip, v7_strip, v8_strip): a strip of 64 rows on one wave, lane
//     t owning row m0 + t one column behind lane t-1, the strip above followed through a progress word, the last row flushed
//     to HBM for the strip below.  The waits and publishes (StripSync), the hand-over of lane 0's upper
//     neighbours, and the queue pop / dead-DP release of the persistent kernels exist once, here; what the
//     kernels do differently on purpose is spelled out in their traits (StripTraits below).
// A kernel file keeps what is particular to it: record layout, LDS plan, stage_load / stage_store / flush_rows, the cell.
#ifndef G2G_STRIP_H
#define G2G_STRIP_H

// ======================================================== 1. primitives ========================================================
// Everything below lives in LDS and says so in its pointer types (address space 3): generic pointers
// would compile to flat_load/flat_store instead of ds_read/ds_write.
#define LDS __attribute__((address_space(3)))
typedef LDS char lchar;
typedef LDS unsigned lu32;
typedef LDS int li32;
typedef LDS double lf64;

// HBM pointers of the sweep carry their address space: a generic pointer compiles to flat_load/flat_store, which also
// occupy the LDS counter (every wait for an LDS read would then wait for the global loads in flight as well)
#define GLB __attribute__((address_space(1)))
template <class T> __device__ __forceinline__ const GLB T *glb(const T *p) { return (const GLB T *) p; }
template <class T> __device__ __forceinline__ GLB T *glbw(T *p) { return (GLB T *) p; }

// ---- bounded waits on progress words of other resident workgroups -------------------------------------------------------
// Persistent workgroups poll flags / progress counters that other workgroups of the SAME launch write.  Dependencies sit
// earlier in the queue than their dependents, so a wait can only be long, not endless -- unless something outside the design
// happens (several processes oversubscribing the device were seen to stretch waits past an iteration-count bound).  The
// bound is therefore WALL CLOCK (s_memrealtime: 100 MHz, keeps running while a wave is descheduled), set per launch by the
// host (hdr[3], units of 65536 ticks = 0.655 ms), and a time-out costs ONE DP, not the batch: the DP is marked in the
// batch's fail array, every other wait of that DP gives up at its next check, its remaining strips are skipped, and
// g2g_batch_run re-runs the marked DPs (on the ordinary kernels once more, then on the non-polling g2g_forward_kernel).
// hdr = done + G2G_HDR: [0] time-outs, [1] strip index of the first, [2] offset of the fail array from `done`, [3] the limit,
// [4..47] what the first wave to give up saw (the host prints it under G2G_WARN; DESIGN.md 4.2 reads such reports).
#define G2G_HDR 24                   // d_flags: [0, 24) queue heads of the kernel variants, [24, 28) this header, [28, 72) snapshot of the first time-out, tile flags behind
// Two 128-byte lines per strip.  The FIRST holds the progress word and nothing else: it is the line other workgroups poll, and the
// only store that ever goes into it is the publish itself.  Everything the strip leaves for a time-out report (HW_ID, markers,
// per-wave columns, heartbeats) lives in the SECOND line, G2G_DIAG ints on, which nobody polls.  Round 4's reports showed what the
// stopped workgroups of DESIGN.md 4.2 were doing: the head strip of every pipeline of one launch sat at an s_waitcnt vmcnt(0)
// behind a write-through store INTO THE LINE ITS SUCCESSOR WAS POLLING (its queue marker, its per-wave column, the progress
// word itself), for as long as the polling went on -- a store starved by a stream of coherent loads from another XCD.  Hence
// also G2G_POLL / G2G_POST: with -DG2G_POLL_RMW the progress word is read and written with read-modify-write atomics, which
// execute at the memory side and leave no copy of the line in anybody's L2.  MEASURED (three whole refinements each way, round
// 4): the events went on with both remedies in place (1, 1 and 3 per run), and the RMW polls cost 4 % -- the hypothesis is refuted,
// the split lines stay (they cost nothing), the polls and publishes are plain agent-scope loads and stores again.
#include "g2g_lds.h"                 // G2G_FSTRIDE (ints between two tile flags / progress words), G2G_HDRN, G2G_DUMP_STRIPS / _WORDS: the host plans with them
#define G2G_DIAG 32                  // offset of a strip's diagnostics line from its progress word
#ifdef G2G_POLL_RMW
#define G2G_POLL(p) __hip_atomic_fetch_or((int *) (p), 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define G2G_POST(p, v) ((void) __hip_atomic_exchange((int *) (p), (int) (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
#else
#define G2G_POLL(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define G2G_POST(p, v) __hip_atomic_store((int *) (p), (int) (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#endif
#define G2G_GAP_TICKS 400000ull       // 4 ms of s_memrealtime: more than ten times what 64 polls take
__device__ __forceinline__ int g2g_wait_ge(const int *p, const int want, int *hdr, int *failp, const int slot)
{
    int v = G2G_POLL(p);
    if (v >= want) return v;
    // The limit counts the time THIS wave was running: a gap of more than G2G_GAP_TICKS between two looks at the clock (64 polls:
    // 0.3 ms when the wave runs) means the wave itself was off the machine -- and with it, as a rule, the rest of its kernel, the
    // producer included -- so only G2G_GAP_TICKS of it count.  Gaps are counted in hdr[40] (longest, in units of 1024 ticks, in
    // hdr[41]): the host reports them whether or not a wait was lost.
    unsigned long long tl = __builtin_amdgcn_s_memrealtime(), run = 0;
    for (unsigned it = 1; ; ++it) {
        // back off: the first polls come 0.2 us apart, later ones 2-3 us with a phase that differs from wave to wave (hundreds of
        // waits per sweep last tens of ms -- strips pulled long before their producers get going: no point in hammering the fabric)
        const unsigned nap = it < 16 ? 1 : it < 64 ? 2 + (it & 1) : 8 + ((it * 5 + (unsigned) slot) & 7);
        for (unsigned j = 0; j < nap; ++j) __builtin_amdgcn_s_sleep(8);
        v = G2G_POLL(p);
        if (v >= want) return v;
        if ((it & 63) == 0) {
            if (__hip_atomic_load(failp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {                       // this DP is lost already
                // ... and this wave was waiting too: of all the waves released this way the one with the LOWEST strip index leaves what
                // it was waiting for and what it last saw (the blocker of its DP, if the blocker itself sat in a wait)
                const int key = 0x7fffffff - slot;
                if (key > atomicMax(hdr + 72, key)) {
                    hdr[73] = want; hdr[74] = v; hdr[75] = (int) (p - (hdr - G2G_HDR)); hdr[76] = (int) it; hdr[77] = (int) (run >> 16);
                    hdr[78] = atomicAdd((int *) p, 0);
                }
                return 0x7fffffff;
            }
            const unsigned long long tn = __builtin_amdgcn_s_memrealtime();
            unsigned long long d = tn - tl;
            tl = tn;
            if (d > G2G_GAP_TICKS) {
                atomicAdd(hdr + 40, 1);
                atomicMax(hdr + 41, (int) (d >> 10 > 0x7fffffffull ? 0x7fffffffull : d >> 10));
                d = G2G_GAP_TICKS;
            }
            run += d;
            if ((run >> 16) > (unsigned long long) (unsigned) __hip_atomic_load(hdr + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                __hip_atomic_store(failp, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                {   // where the waves that gave up sit, and where their producers sit (v6 strips leave HW_ID / XCC_ID next to their progress word)
                    const int my_xcc = (int) __builtin_amdgcn_s_getreg((31 << 11) | 20) & 15;
                    const int pr_xcc = __hip_atomic_load(p + G2G_DIAG + 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    atomicAdd(hdr + 24 + (my_xcc & 7), 1);
                    if ((pr_xcc & ~15) == 0x100) atomicAdd(hdr + 32 + (pr_xcc & 7), 1);
                }
                if (atomicAdd(hdr, 1) == 0) {
                    hdr[20] = __hip_atomic_load(p + G2G_DIAG + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    hdr[21] = __hip_atomic_load(p + G2G_DIAG + 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    hdr[22] = (int) __builtin_amdgcn_s_getreg((31 << 11) | 4);
                    hdr[23] = (int) __builtin_amdgcn_s_getreg((31 << 11) | 20);             // the first one leaves a snapshot for the host's report
                    hdr[1] = slot; hdr[4] = want; hdr[5] = v;
                    const int off = (int) (p - (hdr - G2G_HDR));
                    hdr[6] = off; hdr[7] = (int) (failp - (hdr - G2G_HDR));
                    for (int k = 0; k < 8 && off - k * G2G_FSTRIDE >= G2G_HDR + G2G_HDRN; ++k) hdr[8 + k] = __hip_atomic_load(p - k * G2G_FSTRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    // the producer's heartbeat (v6 strips: step counter and a marker of the place in the step, stored next to the
                    // progress word), read twice 50 us apart: is the producer running, and where?
                    hdr[16] = __hip_atomic_load(p + G2G_DIAG + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    hdr[17] = __hip_atomic_load(p + G2G_DIAG + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    for (int w = 0; w < 8; ++w) hdr[56 + w] = __hip_atomic_load(p + G2G_DIAG + 12 + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    for (int k = 0; k < 256; ++k) __builtin_amdgcn_s_sleep(8);
                    hdr[18] = __hip_atomic_load(p + G2G_DIAG + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    hdr[19] = __hip_atomic_load(p + G2G_DIAG + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    for (int w = 0; w < 4; ++w) hdr[42 + w] = __hip_atomic_load(p + G2G_DIAG + 8 + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the producer's waves at their last publish (v2 / v3 strips)
                    // per-wave heartbeats of a v2 / v3 producer (builds with -DG2G_HEARTBEAT: (step, place) of each of its waves,
                    // G2G_HB below), read now and once more behind the 50 us above: which wave stands still, and where
                    for (int w = 0; w < 8; ++w) hdr[48 + w] = hdr[56 + w];
                    for (int w = 0; w < 8; ++w) hdr[56 + w] = __hip_atomic_load(p + G2G_DIAG + 12 + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    {   // the BLOCKER: walk down the strips of this DP from the polled word while they have not published anything in this
                        // generation; the lowest such strip has a finished strip (or the top chain) above it -- it waits for nobody's
                        // progress, so where IT stands is the question.  Its markers (v2 strips): +5 taken from the queue by workgroup
                        // (0x20000 | id), +6 past the wait for the left chain, +7 past the first look at the strip above.
                        int kb = 0;
                        const int gen_now = want & ~0xFFFFF;
                        for (int k = 1; k < 64 && off - k * G2G_FSTRIDE >= G2G_HDR + G2G_HDRN; ++k) {
                            const int w = __hip_atomic_load(p - k * G2G_FSTRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            if (w >= (gen_now | 1)) break;            // published something in this generation
                            kb = k;
                        }
                        const int *q = p - kb * G2G_FSTRIDE;
                        hdr[64] = kb;
                        hdr[65] = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        for (int w = 0; w < 5; ++w) hdr[66 + w] = __hip_atomic_load(q + G2G_DIAG + 3 + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        hdr[71] = __hip_atomic_load(q + G2G_DIAG + 8, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    // sweep mode with the chains in the queue: the two chain words of this DP sit right below its first strip's word
                    if (off - (slot + 1) * G2G_FSTRIDE >= G2G_HDR + G2G_HDRN) {
                        hdr[80] = __hip_atomic_load(p - slot * G2G_FSTRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);          // left chain
                        hdr[81] = __hip_atomic_load(p - (slot + 1) * G2G_FSTRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);    // top chain
                    }
                    {   // the whole pipeline above this waiter (the strips' lines are contiguous, the one above p at p - G2G_FSTRIDE): word,
                        // HW_ID, the three markers, the two waves' last publish -- the host finds the strips that wait for nobody in it
                        const int doff = __hip_atomic_load(hdr + 82, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (doff > 0) {
                            int *dump = (hdr - G2G_HDR) + doff;
                            int nd = 0;
                            for (int k = 0; k < G2G_DUMP_STRIPS && k < slot && off - k * G2G_FSTRIDE >= G2G_HDR + G2G_HDRN; ++k) {
                                const int *q = p - k * G2G_FSTRIDE;
                                int *d = dump + 2 + G2G_DUMP_WORDS * k;
                                d[0] = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                d[1] = __hip_atomic_load(q + G2G_DIAG + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                d[2] = __hip_atomic_load(q + G2G_DIAG + 5, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                d[3] = __hip_atomic_load(q + G2G_DIAG + 6, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                d[4] = __hip_atomic_load(q + G2G_DIAG + 7, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                d[5] = __hip_atomic_load(q + G2G_DIAG + 8, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                d[6] = __hip_atomic_load(q + G2G_DIAG + 9, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                for (int w = 0; w < 4; ++w) d[7 + w] = __hip_atomic_load(q + G2G_DIAG + 12 + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (-DG2G_HEARTBEAT: step / place of the strip's two waves)
                                nd = k + 1;
                            }
                            dump[0] = nd; dump[1] = slot;
                        }
                    }
                    hdr[8 + 38] = atomicAdd((int *) p, 0);          // the same word through a read-modify-write (executes at the coherent point)
                    hdr[8 + 39] = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                return 0x7fffffff;
            }
        }
    }
}
__device__ __forceinline__ bool g2g_dp_failed(const int *failp) { return __hip_atomic_load(failp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0; }
// Strip-boundary records cross workgroups (and XCDs: each has its own L2).  Plain accesses ordered by agent-scope release /
// acquire fences cost a write-back of the whole L2 (buffer_wbl2) per publish and an invalidate (buffer_inv) per consumed
// publish -- from hundreds of workgroups, every few steps when a handful of DPs publish every 4 steps (g2g_refine's windows).
// The records themselves are therefore written with agent-scope (write-through) stores and read with agent-scope loads, and
// publishing is: wait for the stores, store the progress word -- no cache-maintenance operation in the step loop.  Measured
// speed-neutral; adopted because the producers that were seen to stop stopped where a wave
// can only be waiting for its own memory operations.  -DG2G_FENCE restores the fenced form.
#ifndef G2G_FENCE
#define G2G_NOFENCE 1
#endif
#ifdef G2G_NOFENCE
#define G2G_XLD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define G2G_XST(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define G2G_ACQUIRE()
#define G2G_RELEASE()
#else
#define G2G_XLD(p) (*(p))
#define G2G_XST(p, v) (*(p) = (v))
#define G2G_ACQUIRE() __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent")
#define G2G_RELEASE() __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent")
#endif
// Passive producer-side heartbeat of the v2 / v3 strips (build with G2G_EXTRA_FLAGS=-DG2G_HEARTBEAT, which also turns on the v6
// strips' G2G_V6_HEARTBEAT): every wave of a strip keeps (step, place in the step) in words 12 + 2 w / 13 + 2 w of the strip's
// progress line; whoever times out waiting for the strip copies them into its report twice, 50 us apart (g2g_wait_ge,
// hdr[48..63]) -- the report then names the wave that stands still and the place it stands at.  Off by default: a handful of
// write-through stores per step and wave.  Places (v2): 1 top of the step, 2 publish entered, 3 behind the publish barrier,
// 4 waiting for the strip above, 5 behind the column-score block, 6 sources staged, 7 cell done, 8 at the step's barrier.
#ifdef G2G_HEARTBEAT
#define G2G_HB_STEP(pself, w, s) { if (pself) __hip_atomic_store((pself) + G2G_DIAG + 12 + 2 * (w), (int) (s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#define G2G_HB(pself, w, k) { if (pself) __hip_atomic_store((pself) + G2G_DIAG + 13 + 2 * (w), (int) (k), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#else
#define G2G_HB_STEP(pself, w, s)
#define G2G_HB(pself, w, k)
#endif

__device__ __forceinline__ void team_sync()
{   // lanes of a team live in one wave: ordering LDS traffic between phases is a compiler matter only
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// progress of a boundary chain that runs as a queue entry of a persistent kernel (sweep mode): same counter format as a
// strip's (g2g_kernels_v3.hip); called by the walking lane after its stores
__device__ __forceinline__ void chain_publish(int *prog, int penc, int v)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    G2G_POST(prog, penc | (v < 0xFFFFF ? v : 0xFFFFF));
}

// ---- a wave-uniform private copy of the DP descriptor -------------------------------------------------
// The descriptor lives in HBM next to buffers the kernel writes, so the compiler must assume every store may
// change it: left alone, the sweep re-reads its fields with vector loads -- and a full vmcnt(0) wait -- in the
// middle of every step.  The fields the sweep uses are therefore copied once per tile into scalar registers.
__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ double uni(double x)
{
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)), __builtin_amdgcn_readfirstlane(__double2loint(x)));
}
template <class T> __device__ __forceinline__ T *uni(T *p)
{
    const unsigned long long v = (unsigned long long) p;
    const unsigned lo = (unsigned) __builtin_amdgcn_readfirstlane((int) (unsigned) v);
    const unsigned hi = (unsigned) __builtin_amdgcn_readfirstlane((int) (unsigned) (v >> 32));
    return (T *) (((unsigned long long) hi << 32) | lo);
}
__device__ __forceinline__ void uni_side(DevSide &d, const DevSide &s)
{
    d.many = uni(s.many); d.len = uni(s.len); d.left = uni(s.left); d.right = uni(s.right); d.nils = uni(s.nils);
    d.nelm = uni(s.nelm); d.felm = uni(s.felm); d.hetero = uni(s.hetero); d.maxlist = uni(s.maxlist);
    d.seq = uni(s.seq); d.weight = uni(s.weight); d.pseq = uni(s.pseq); d.thk = uni(s.thk);
    for (int v = 0; v < 3; ++v) { d.off[v] = uni(s.off[v]); d.glen[v] = uni(s.glen[v]); d.freq[v] = uni(s.freq[v]); }
    d.gapdens = uni(s.gapdens); d.postgapdens = uni(s.postgapdens);
}
__device__ __forceinline__ void uni_prob(DevProb &d, const DevProb &s)
{
    d.kind = uni(s.kind); d.noll = uni(s.noll); d.sim2_kind = uni(s.sim2_kind); d.crg2_kind = uni(s.crg2_kind);
    d.codonk1 = uni(s.codonk1); d.lw = uni(s.lw); d.up = uni(s.up); d.width = uni(s.width);
    d.basic_gop = uni(s.basic_gop); d.weighted_gop = uni(s.weighted_gop); d.u = uni(s.u);
    d.u2divu1 = uni(s.u2divu1); d.v2divv1 = uni(s.v2divv1);
    d.simmtx = uni(s.simmtx); d.simdim = uni(s.simdim); d.capa = uni(s.capa); d.capb = uni(s.capb);
    uni_side(d.a, s.a); uni_side(d.b, s.b);
    d.v2_rowH = uni(s.v2_rowH); d.v2_rowG = uni(s.v2_rowG); d.v2_rowG2 = uni(s.v2_rowG2); d.v2_colH = uni(s.v2_colH);
    d.v2_cbH = uni(s.v2_cbH); d.v2_cbF = uni(s.v2_cbF); d.v2_cbF2 = uni(s.v2_cbF2);
    d.v2_rowstride = uni(s.v2_rowstride); d.v2_sim = uni(s.v2_sim); d.v2_rowoff = uni(s.v2_rowoff);
    d.trace = uni(s.trace); d.tstride = uni(s.tstride); d.d0 = uni(s.d0); d.d1 = uni(s.d1);
    d.score = uni(s.score);
}

// ---- strip-local column scores (sweep mode) ----------------------------------------------------------------------
// PwdM::sim2 of a cell does not depend on the recurrence.  Tile mode reads it from a matrix a separate kernel fills ahead
// of the sweep (8 B per cell of HBM, written once and read once).  A strip in sweep mode makes its own instead, block by
// block: every 64 steps it computes the (rows of the strip) x 64 columns its first row enters 64 steps later -- thread <->
// column, rows in a loop, so a row's profile vector is a wave-uniform read and the stores are coalesced -- into one of
// THREE 32 KB buffers of a per-workgroup scratch area (the rows of a skewed strip straddle two blocks while the third is
// filled).  The scratch area is reused by every strip the workgroup runs: ~100 MB per launch, cache resident, instead of
// 8 B per cell of the sweep.
#define GLBV3 __attribute__((address_space(1)))
#ifndef G2G_SIMBLK_STRIDE
#define G2G_SIMBLK_STRIDE (3 * 4096)          // doubles of column-score scratch per workgroup: three blocks of 64 x 64
#endif
struct SimBlk { GLBV3 double *buf; int cbase; };
// (tid / nthr / rows: the filling threads -- one wave for the one-lane-per-cell kernels, the workgroup for v2 -- and the
// rows of a strip; thread <-> column tid & 63, rows tid >> 6, tid >> 6 + nthr / 64, ...)
__device__ __forceinline__ void simblk_fill(const DevProb &P, const SimBlk &S, const int bk, const int m0, const int tid,
                                            const int nthr = 64, const int rows = 64)
{
    const int n = S.cbase + bk * 64 + (tid & 63);
    if (bk < 0 || n >= P.b.right) return;
    GLBV3 double *dst = S.buf + (size_t) (bk % 3) * 4096 + (tid & 63);
    for (int r = tid >> 6; r < rows; r += nthr >> 6) {
        const int m = m0 + r;
        if (m >= P.a.right) break;
        int nlo = m + P.lw; if (nlo < P.b.left) nlo = P.b.left;
        int nhi = m + P.up + 1; if (nhi > P.b.right) nhi = P.b.right;
        if (n >= nlo && n < nhi) dst[r * 64] = sim2(P, m, n);
    }
}
// The same block through the block scorer (sim2_block, g2g_kernels.hip): one scorer dispatch per block, the column's operands
// in registers, one memory wait per row or per eight elements instead of one or two per element.  v6 fills its blocks with it
// (one wave per SIMD: nobody hides a wait).  The other strip families stay on simblk_fill: with the block scorer inlined their
// register allocation loses more than the fill gains (scratch of g2g_v3r_hf2 256 -> 304 B, of g2g_v2_hf3 8 -> 1120 B, and
// g2g_v3r_hf2, whose sweep DPs read sim31 in place and never fill a block, 134.5 -> 143.7 ms per sweep).
__device__ __forceinline__ void simblk_fill_block(const DevProb &P, const SimBlk &S, const int bk, const int m0, const int tid,
                                                  const int nthr = 64, const int rows = 64)
{
    const int n0 = S.cbase + bk * 64;
    if (bk < 0 || n0 >= P.b.right) return;                 // (the whole block: every wave takes the same way)
    SimRows R;                                             // sim2_block (g2g_kernels.hip): one scorer dispatch per block, all lanes active
    R.lane = tid & 63;
    asm volatile("" : "+v"(R.lane));                       // (nothing derived from the lane is hoisted out of the step loop into registers the cell needs)
    R.n = n0 + R.lane; R.nn = R.n < P.b.right ? R.n : P.b.right - 1;
    R.dst = S.buf + (size_t) (bk % 3) * 4096 + R.lane;
    R.m0 = m0;
    asm volatile("" : "+s"(R.m0));                         // (... nor anything derived from the strip's first row into SGPRs: g2g_v6_pf3 has neither to spare)
    R.r0 = __builtin_amdgcn_readfirstlane(tid >> 6); R.rstep = nthr >> 6; R.rows = rows;
    sim2_block(P, R);
}
__device__ __forceinline__ const GLBV3 double *simblk_at(const SimBlk &S, const int row, const int n)
{
    const int k = n - S.cbase;
    return S.buf + (size_t) ((k >> 6) % 3) * 4096 + row * 64 + (k & 63);
}

struct RS { double val; int dir, glb; };                  // record scalars
__device__ __forceinline__ RS rs_black() { RS r; r.val = NEVSEL; r.dir = 0; r.glb = 0; return r; }
// lane t <- lane t-1 over the whole wave: one DPP move per dword (wave_shr:1), no LDS crossbar round trip
__device__ __forceinline__ int dpp_up1(int x) { return __builtin_amdgcn_update_dpp(0, x, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ RS rs_up(const RS &x)
{
    RS r;
    r.val = __hiloint2double(dpp_up1(__double2hiint(x.val)), dpp_up1(__double2loint(x.val)));
    r.dir = dpp_up1(x.dir); r.glb = dpp_up1(x.glb);
    return r;
}
__device__ __forceinline__ RS rs_sel(bool c, const RS &x, const RS &y)
{
    RS r; r.val = c ? x.val : y.val; r.dir = c ? x.dir : y.dir; r.glb = c ? x.glb : y.glb; return r;
}

// ring slots: H corner c -> c mod 3 (0..2); G corner c -> 3 + (c & 1); F -> 5; G2 -> 6 + (c & 1); F2 -> 8
__device__ __forceinline__ int mod3(int c) { return ((c % 3) + 3) % 3; }
#define SLOT_H(c) (mod3(c))
#define SLOT_G(c) (3 + ((c) & 1))
#define SLOT_F 5
#define SLOT_G2(c) (6 + ((c) & 1))
#define SLOT_F2 8

// ======================================================== 2. the scaffold ======================================================
// What the strip kernels do differently on purpose, by name.  The defaults are what v7 / v8 do; V3Strip, V6Strip and V7Strip
// (next to their strip functions) override the rest.  v3 and v6 also call strip_where, v7 and v8 do not.  Nothing is unified
// here: what a kernel leaves for the stall report is a decision of its own.
// NOT here yet: the strip geometry (m0 ... llo), the wait on the left chain, the trace index and the pl / pu lines of the kernel
// loops are still written out per file.  Every shared form of them that was tried changed the register allocation of
// g2g_v3r_hf2 / g2g_v6_pf2; what is here compiles to the code the per-file copies compiled to.
struct StripTraits {
    static constexpr bool PUB_COL = false;                 // publish leaves its column in G2G_DIAG + 8 (v3, as the v2 strips)
    static constexpr bool REC_GLB = true;                  // staged records carry glb in dword 3 (v7: no gap state, reads 0)
    static __device__ __forceinline__ void acquire() { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); }
    static __device__ __forceinline__ void release() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); }
    static __device__ __forceinline__ void mark(int *, int) {}            // place marker inside publish (v6 heartbeat builds)
};

// ---- the strip's progress words: the strip above (prog_up), its own (prog_self), the report header and the DP's fail flag
struct StripSync { const int *prog_up; int *prog_self, *dbg, *failp; int penc, avail, ti; };
__device__ __forceinline__ StripSync strip_sync(const int *prog_up, int *prog_self, int *dbg, int *failp, const int pgen, const int ti)
{   // avail: corner columns of the strip above known to be final
    const StripSync S = {prog_up, prog_self, dbg, failp, (pgen & 0x7FF) << 20, prog_up ? 0 : 0x7fffffff, ti};
    return S;
}
template <class T>
__device__ __forceinline__ void strip_need(StripSync &S, const int col)       // wave-uniform: every lane polls, nobody branches alone
{
    const int want = S.penc | (col < 0xFFFFF ? col : 0xFFFFF);
    if (S.prog_up && want > S.avail) {
        S.avail = g2g_wait_ge(S.prog_up, want, S.dbg, S.failp, S.ti);
        T::acquire();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
}
template <class T>
__device__ __forceinline__ void strip_publish(const StripSync &S, const int col)      // corners <= col of this strip's last row are in HBM
{
    if (S.prog_self) {
        T::mark(S.prog_self, 9);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        T::mark(S.prog_self, 10);
        T::release();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        T::mark(S.prog_self, 11);
        if (T::PUB_COL) __hip_atomic_store(S.prog_self + G2G_DIAG + 8, col, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (the wave's last publish, for the time-out report)
        G2G_POST(S.prog_self, S.penc | (col < 0 ? 0 : col < 0xFFFFF ? col : 0xFFFFF));
        T::mark(S.prog_self, 12);
    }
}
// where this strip runs: for the time-out report of whoever waits for it (g2g_wait_ge)
__device__ __forceinline__ void strip_where(const StripSync &S)
{
    if (S.prog_self) {
        __hip_atomic_store(S.prog_self + G2G_DIAG + 3, (int) __builtin_amdgcn_s_getreg((31 << 11) | 4), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(S.prog_self + G2G_DIAG + 4, 0x100 | ((int) __builtin_amdgcn_s_getreg((31 << 11) | 20) & 15), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- hand-over from the strip above: lane 0's diagonal and upper neighbours at lane 0's column n0 come from the staging
// scalars (stsc: H ring 0-2, G 3-4, G2 5-6, four dwords each), every other lane keeps what DPP handed down
template <class T>
__device__ __forceinline__ RS strip_staged(const lu32 *q)
{
    RS t; t.val = *(const lf64 *) q; t.dir = (int) q[2]; t.glb = T::REC_GLB ? (int) q[3] : 0; return t;
}
template <class T, bool NOLL3>
__device__ __forceinline__ void strip_handover(const lu32 *stsc, const int n0, const int lane, RS &hd, RS &hu, RS &gu, RS &g2u)
{
    hd = rs_sel(lane == 0, strip_staged<T>(stsc + SLOT_H(n0) * 4), hd);
    hu = rs_sel(lane == 0, strip_staged<T>(stsc + SLOT_H(n0 + 1) * 4), hu);
    gu = rs_sel(lane == 0, strip_staged<T>(stsc + (3 + ((n0 + 1) & 1)) * 4), gu);
    if (NOLL3) g2u = rs_sel(lane == 0, strip_staged<T>(stsc + (5 + ((n0 + 1) & 1)) * 4), g2u);
}

// ---- the persistent kernels' loop (V2_KERNEL ... V8_KERNEL).  NOTE on control flow: see V2_KERNEL -- everything here is
// executed uniformly by every lane.  Each kernel keeps ONE call site of its strip function (see V3_KERNEL).
// queue pop: each thread adds (tid == 0) to the queue head, parks its result in LDS, slot 0 is the tile
__device__ __forceinline__ int strip_pop(int *qhead, li32 *s_vals)
{
    s_vals[threadIdx.x] = atomicAdd(qhead, threadIdx.x == 0 ? 1 : 0);
    __syncthreads();
    const int t = __builtin_amdgcn_readfirstlane(s_vals[0]);
    __syncthreads();
    return t;
}
__device__ __forceinline__ int strip_done_word(const int gen) { return ((gen & 0x7FF) << 20) | 0xFFFFF; }
// did this DP lose a wait?  Then its strips are skipped and strip_release posts `post` into their words for the dependents
__device__ __forceinline__ int strip_dp_dead(const int *failp, li32 *s_vals)
{
    if (threadIdx.x == 0) s_vals[0] = g2g_dp_failed(failp) ? 1 : 0;      // (one reader: the branch must be uniform)
    __syncthreads();
    const int dp_dead = s_vals[0];
    __syncthreads();
    return dp_dead;
}
__device__ __forceinline__ void strip_release(int *self, const int post)
{
    if (threadIdx.x == 0) G2G_POST(self, post);
    __syncthreads();
}
#endif
