/*
 * g2g.h -- C ABI of the MI355X-native group-to-group alignment DP (libg2g.so).
 *
 * Drop-in boundary for ONE hot path of ogotoh/prrn_aln: the group-to-group affine / double-affine gap
 * DP that align2() dispatches to (reference src/maln2.cc:1875 -> alignC<recd_t> src/fwd2c.h:671 ->
 * Fwd2c<recd_t>::forwardB src/fwd2c.h:359 + Vmf::traceback src/vmf.cc:105 + stdskl src/gaps.cc:139).
 * Plain pointers and sizes only; no C++/torch types.  Every entry point names the reference interface
 * it replaces.  All scores are IEEE-754 doubles (the prrn build: -DDVAL=1, reference src/cmn.h:40-50).
 *
 * Two levels:
 *   level 1 ("operator")  g2g_group / g2g_pwdm / g2g_align2      <-> mSeq / PwdM / align2()
 *   level 0 ("engine")    g2g_problem / g2g_forward_batch        <-> Fwd2c<recd_t>(seqs,pwd).forwardB()+traceback()
 * Level 1 builds a g2g_problem on the host (mode selection, thickness, profile vectors, gap profiles:
 * SURVEY.md §8 rows a7-a9) and hands it to level 0, which runs on the GPU.  There is no CPU fallback:
 * if no HIP device is usable every compute entry point returns G2G_ERR_NODEVICE.
 */
#ifndef G2G_H_
#define G2G_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define G2G_ABI_VERSION 5

/* error codes (negative) */
enum {
    G2G_OK              =  0,
    G2G_ERR_ARG         = -1,   /* malformed argument                                            */
    G2G_ERR_MODE        = -2,   /* alignment mode not on this path (spliced _ALS/_ALH, ether u0>0, SSHP):
                                   the reference itself would fatal() (maln2.cc:1918) or use Fwd2h/Fwd2s */
    G2G_ERR_NODEVICE    = -3,   /* no usable HIP device / kernel image                           */
    G2G_ERR_DEVICE      = -4,   /* HIP runtime error (message via g2g_last_error)                */
    G2G_ERR_NOMEM       = -5,
    G2G_ERR_ENDS        = -6    /* skeleton ends mismatch even at sh = -100 (maln2.cc:1946-1952) */
};

/* reference enum ALN_MODE, src/aln.h:71-76 (banded "_ALB" = default because algmode.bnd = 1) */
enum {
    G2G_NGP_ALN = 1, G2G_HLF_ALN = 2, G2G_RHF_ALN = 3, G2G_GPF_ALN = 4, G2G_NTV_ALN = 5,
    G2G_NGP_ALB = 6, G2G_HLF_ALB = 7, G2G_RHF_ALB = 8, G2G_GPF_ALB = 9, G2G_NTV_ALB = 10
};

/* which PwdM::sim?? column scorer (reference src/maln.h:159-173,205-209; table maln2.cc:347-399).
   value = 10*kind + (weighted ? 1 : 0) for the member-loop scorers */
enum {
    G2G_SIM00 = 0, G2G_SIM11 = 11, G2G_SIM12I = 120, G2G_SIM12W = 121, G2G_SIM13 = 13,
    G2G_SIM21I = 210, G2G_SIM21W = 211, G2G_SIM22I = 220, G2G_SIM22W = 221,
    G2G_SIM23I = 230, G2G_SIM23W = 231, G2G_SIM31 = 31, G2G_SIM32I = 320, G2G_SIM32W = 321,
    G2G_SIM33 = 33, G2G_SIM33N = 330
};

/* reference enum TraceBackDir, src/aln.h:47-52 (only the values Fwd2c produces) */
enum { G2G_DEAD = 0, G2G_DIAG = 2, G2G_NEWD = 3, G2G_VERT = 4, G2G_HORI = 8, G2G_NEWV = 12, G2G_NEWH = 13 };

/* reference struct SKL {int m, n;}, src/cmn.h:124 */
typedef struct g2g_skl { int32_t m, n; } g2g_skl;

/* ---- level 0: the flattened DP problem -------------------------------------------------------- */

/* Static gap profile of one group: the three views Gfq::sfrq/tfrq/rfrq (reference src/gfreq.h:44-64,
   src/gfreq.cc:247-312).  View v (0 = s, 1 = t, 2 = r): the list of position p (p = -1 .. len-1) is
   glen[v][off[v][p+1] ...], ascending in glen and terminated by an entry with glen = -1 (the
   terminator is part of the pool).  off[v] has len+2 entries (the last one = pool length).
   freq of the s view is in accumulated (suffix-sum) form, as the reference stores it. */
typedef struct g2g_gapprof {
    int32_t        hetero;          /* Gfq::hetero: capacity of a dynamic gap-state list is hetero+1 */
    const int32_t *off[3];
    const int32_t *glen[3];
    const double  *freq[3];
} g2g_gapprof;

/* One side of the DP as mSeqItr hands it out (reference src/mseq.h:206-350, src/mseq.cc:760-815). */
typedef struct g2g_side {
    int32_t        many;            /* members                                                    */
    int32_t        len;             /* columns                                                    */
    int32_t        left, right;     /* range to align, reference Seq::left/right                  */
    int32_t        nils;            /* inex.nils                                                  */
    int32_t        dels;            /* inex.dels (any internal/terminal gap)                      */
    const uint8_t *seq;             /* (len+2)*many residue codes, position -1 first ([pos][member],
                                       reference Seq::at(), nil_code=0 gap_code=1 seq.h:76-77)    */
    const double  *weight;          /* many, or NULL                                              */
    int32_t        nelm, felm;      /* profile vector geometry (mseq.h:53-59); 0 if not vectorised */
    const double  *pseq;            /* (len+2)*nelm, position -1 first, or NULL                   */
    const double  *thk;             /* (len+2)*3 {cfq,dfq,efq} at positions -1..len: SeqThk as the
                                       iterator yields it for each position (thk_mode folded in)  */
    int32_t        has_gfq;
    g2g_gapprof    gfq;             /* valid iff has_gfq                                          */
    /* NTV modes only: per position/member gap densities (mSeq::gapdensity/postgapdensity,
       mseq.h:148-160), (len+2)*many each, position -1 first; NULL otherwise */
    const double  *gapdens;
    const double  *postgapdens;
    /* exon-boundary (intron position) annotation of the group, reference SigII::pfq (src/gsinfo.h:33,41-46): npfq entries
       ascending in pos (nucleotide coordinate: column x pfq_step + phase), dns = weighted number of members with an intron
       there; pfq_step = SigII::step (3 for protein columns, 1 for nucleotides).  npfq = 0 / NULL: not annotated.          */
    int32_t        npfq, pfq_step;
    const int32_t *pfq_pos;
    const double  *pfq_dns;
    double         sumwt;           /* Seq::sumwt: sum of the members' weights (the member count when unweighted); read by the
                                       PwdM::stt?? statistics (van / vbn and the thickness of the zero iterators)          */
    /* ABI 5: device-resident twins of the arrays above (same contents, in the HBM of the context that built them:
       g2g_pwdm_create_batch builds a group's derived arrays on the device and leaves them there).  NULL for a side that lives on
       the host only.  A batch prepared from such a side reads the twins where they lie -- nothing is packed or uploaded for them --
       so the objects that own them (the g2g_group behind the g2g_pwdm) must outlive the batch, like the host arrays. */
    const struct g2g_side_dev *dev;
} g2g_side;
typedef struct g2g_side_dev {
    const struct g2g_ctx *ctx;      /* the twins are addresses in THIS context's device                                      */
    const uint8_t *seq;
    const double  *weight, *pseq, *thk;
    const int32_t *off[3], *glen[3];
    const double  *freq[3];
} g2g_side_dev;

typedef struct g2g_problem {
    int32_t  alnmode;               /* G2G_*_ALB / _ALN                                            */
    int32_t  sim2_kind;             /* G2G_SIM*                                                   */
    int32_t  noll;                  /* PwdB::Noll: 2 affine, 3 double affine (aln2.cc:100)        */
    int32_t  codonk1;               /* PwdB::codonk1 (aln2.cc:116-117)                            */
    int32_t  lw, up;                /* band: WINDOW from stripe() (aln2.cc:156-174)               */
    int32_t  crg2_kind;             /* NTV engines: which PwdM::crg?? (maln2.cc:881-1024,1454-1614):
                                       11, 120/121 (12i/12w), 210/211, 220/221; 0 otherwise         */
    int32_t  dvsp;                  /* PwdB::DvsP: 0 nucleotide x nucleotide (the statistics read compacted codes), 3 protein x protein */
    double   basic_gop;             /* PwdM::Basic_GOP  = -scale*v (maln2.cc:232)                 */
    double   weighted_gop;          /* PwdM::Weighted_GOP = -v     (maln2.cc:237)                 */
    double   u;                     /* alnprm.u, unpaired-column penalty in unp1 (maln.h:185)     */
    double   u2divu1, v2divv1;      /* LongGEP/BasicGEP, LongGOP/BasicGOP (fwd2c.h:85-86)         */
    const double *simmtx;           /* rows x dim substitution matrix, Simmtx::mtx (simmtx.h:49)  */
    int32_t  simdim, simrows;
    g2g_side a, b;
    double   spb_fact;              /* SpbFact = alprm.scale * alprm2.spb (src/gsinfo.cc:35): weight of the intron-position bonus
                                       PfqItr::match_score adds in forwardB (src/fwd2c.h:378-379,446-452,472) when BOTH sides are
                                       annotated; 0 switches it off.  DPs with the bonus run on the bonus-aware strip kernels
                                       (DPunit: v7, _hf / _pf: v2) or on g2g_forward_kernel (_nv, option NO_STRIP_BONUS):
                                       g2g_batch_paths tells which.                                                            */
} g2g_problem;

/* result of one DP */
typedef struct g2g_result {
    double    score;                /* Fwd2c::forwardB return value (= *scr of align2)            */
    int64_t   cells;                /* in-band cells visited: sum_m (n9 - n), fwd2c.h:373-374,393 */
    int32_t   ntrace;               /* records in `trace`                                         */
    int32_t   status;               /* G2G_OK or error for this item                              */
    g2g_skl  *trace;                /* Vmf::traceback(-1) order: end corner first, origin last
                                       (vmf.cc:105-120); free with g2g_free()                     */
    int64_t   rr[2];                /* what forwardB(pp) reports without a Vmf (HomScoreC, fwd2c.h:664-668,
                                       468-469,477-480): diagonal n-m on which the path leaves the first row,
                                       and b.left - a.left + b.right - a.right                      */
} g2g_result;

typedef struct g2g_ctx g2g_ctx;

/* Create a context bound to one HIP device (device < 0: current device).  Returns NULL on failure.
   Threading: a context (its streams, its pinned staging buffer and its pool of device memory) serves ONE host thread at a
   time -- callers with several threads serialise their calls or batch them (integration/g2g_bind.cc does the latter);
   the group / PwdM builders (g2g_group_create, g2g_pwdm_create) touch only their own objects and may run on any
   number of threads.  g2g_last_error() is per thread.  One process per GPU: the persistent kernels poll flags
   written by other resident workgroups of the same launch and must not compete with another process for the device
   (every wait is bounded; an oversubscribed device shows up as a failed batch, not a hang).                       */
g2g_ctx *g2g_create(int device);
void     g2g_destroy(g2g_ctx *ctx);
const char *g2g_last_error(void);
int      g2g_abi_version(void);
/* 1 if a HIP device + gfx950 code object are usable, else 0 (never falls back to the host). */
int      g2g_device_ok(g2g_ctx *ctx);
/* Tuning and diagnostic switches of ONE context (kernel-variant selection, strip widths, the waits' time limit, arena
   limits, debug output: DESIGN.md section 4 lists the names).  `name` is given with or without the "G2G_" prefix.
   A switch the context has not set reads the environment variable G2G_<NAME> (the environment only supplies
   defaults); value == NULL turns a switch off for this context whatever the environment says.  Takes effect at the
   next g2g_batch_prepare / g2g_forward_batch.  g2g_get_option returns the effective value or NULL (valid until the
   next g2g_set_option on the context). */
int         g2g_set_option(g2g_ctx *ctx, const char *name, const char *value);
const char *g2g_get_option(const g2g_ctx *ctx, const char *name);
void        g2g_reset_options(g2g_ctx *ctx);     /* forget every g2g_set_option: back to the environment's defaults */

/* Fwd2c<recd_t>(seqs, pwd, trb=true).forwardB() + traceback() for a batch of independent problems
   (alignC<recd_t>, reference src/fwd2c.h:671-677).  res[i].trace is malloc'ed by the library. */
int      g2g_forward_batch(g2g_ctx *ctx, int n, const g2g_problem *const *prob, g2g_result *res);

/* The same in three steps, for callers that keep a sweep resident in HBM (bench.py times g2g_batch_run
   only: inputs are already in device memory when it starts).  g2g_batch_times() reports the HIP-event
   durations of the forward and backtrack kernels of the last run, measured on the context's stream.
   The problem descriptions (and every array they point to) must stay valid until g2g_batch_free: a DP that loses
   a scheduler wait is packed again from them and re-run inside g2g_batch_run. */
typedef struct g2g_batch g2g_batch;
int       g2g_batch_prepare(g2g_ctx *ctx, int n, const g2g_problem *const *prob, g2g_batch **out);
int       g2g_batch_run(g2g_batch *b);
int       g2g_batch_fetch(g2g_batch *b, g2g_result *res);
void      g2g_batch_times(const g2g_batch *b, float *fwd_ms, float *tb_ms);
long long g2g_batch_cells(const g2g_batch *b);
size_t    g2g_batch_arena_bytes(const g2g_batch *b);
/* Which kernel generation each of the batch's n problems runs on: gen[i] = 1 (g2g_forward_kernel: one workgroup per DP,
   state in HBM), 2 (8-lanes-per-cell strips), 3 (v3 / v3r), 6, 7 or 8; 0 for a problem that was
   refused (g2g_result::status).  After g2g_batch_prepare: the kernel chosen.  After g2g_batch_run: the kernel that
   produced the result g2g_batch_fetch returns -- a DP re-run after a lost wait reports the kernel of its successful
   re-run.  G2G_ERR_ARG for a NULL argument.  (An entry point added without a change of g2g_abi_version.) */
int       g2g_batch_paths(const g2g_batch *b, int32_t *gen);
/* The cells of a problem that receive the intron-position bonus, as g2g_batch_prepare tabulates them (host only, needs no
   device): row-major, n ascending within a row; h is added to H of cell (m, n), mx to its best non-diagonal record.  Writes
   up to cap entries into each non-NULL array and returns the number of cells (0: no bonus), or G2G_ERR_ARG. */
int       g2g_bonus_cells(const g2g_problem *p, int cap, int32_t *m, int32_t *n, double *h, double *mx);
/* The scheduler's waits are bounded by wall clock: a wait that runs into the limit costs its DP a re-run
   inside g2g_batch_run, and the results stay complete.  These two make every such event visible: for the LAST run of a
   batch the number of waits that gave up and of DPs re-run (and the DPs re-run over the batch's life); for a context
   out[0] = batch runs, out[1] = waits that gave up, out[2] = DPs re-run, out[3] = of those, DPs that needed the
   non-polling kernel -- counted over every entry point that runs DPs (g2g_align2_batch, g2g_refine, ...).  An ordinary
   run reports zeros. */
void      g2g_batch_recovery(const g2g_batch *b, int *timeouts_last_run, int *recovered_last_run, int *recovered_total);
void      g2g_ctx_counters(const g2g_ctx *ctx, long long out[4]);
/* the report of the context's last recovered time-out (which DPs on which kernel, what the first waiting wave saw and where
   its producer ran): "" if there was none; valid until the next event or g2g_destroy */
const char *g2g_ctx_last_timeout(const g2g_ctx *ctx);
/* The waits count the time the waiting wave itself was running: a wave that finds more than 4 ms between two looks at the clock
   was off the machine (with, as a rule, the rest of its kernel) and counts 4 ms of it.  count = such gaps seen by waiting
   waves since g2g_create, longest_ms = the longest: zeros on an undisturbed device. */
void      g2g_ctx_wait_gaps(const g2g_ctx *ctx, long long *count, double *longest_ms);
/* The same over the whole PROCESS (every context, also destroyed ones): out[0] = batch runs, [1] = waits that gave up, [2] = DPs
   re-run, [3] = of those on the non-polling kernel, [4] = gaps seen by waiting waves, [5] / [6] = the part of [1] / [2] that
   came from batches prepared with the INJECT_STALL test hook, [7] reserved.  A host (or a test session: tests/conftest.py)
   that wants a recovery to be an ERROR rather than a counter compares [2] with [6] at its end.  g2g_process_last_timeout copies
   the report of the last event that was NOT injected into buf (NUL-terminated, truncated to cap) and returns its full length. */
void      g2g_process_counters(long long out[8]);
size_t    g2g_process_last_timeout(char *buf, size_t cap);
/* Device memory is owned by the context (a pool of blocks that batches take from and give back to): out[0] = hipMalloc calls
   made for it since g2g_create, [1] = hipFree calls, [2] = requests served from the pool, [3] = bytes free in the pool now.
   A steady-state loop (a refinement: one batch per window) shows [0] standing still. */
void      g2g_ctx_mem_counters(const g2g_ctx *ctx, long long out[4]);
void      g2g_batch_free(g2g_batch *b);

/* stdskl(): sort + normalise a raw traceback into ascending unique corners (reference src/gaps.cc:139).
   in[0..n) raw records; returns malloc'ed corners (count in *nout), caller g2g_free()s. */
g2g_skl *g2g_stdskl(const g2g_skl *in, int n, int *nout);

void     g2g_free(void *p);

/* ---- level 1: the operator surface ------------------------------------------------------------- */

/* subset of reference struct ALPRM (src/seq.h:27-28) + the algmode bits this path reads */
typedef struct g2g_params {
    double  u, v, u0, u1, tgapf, scale, gamma;
    int32_t k1, ls, sh;
    int32_t banded;                 /* algmode.bnd                                                */
    int32_t molc;                   /* 1 PROTEIN, 2 DNA (cmn.h:107)                               */
    const double *simmtx;           /* rows x dim                                                  */
    int32_t simdim, simrows;
    int32_t max_code;               /* SEQ_CODE::max_code of the alphabet                         */
} g2g_params;

typedef struct g2g_group g2g_group;   /* <-> mSeq  */
typedef struct g2g_pwdm  g2g_pwdm;    /* <-> PwdM  */

/* <-> aggregate()/mSeq construction (src/mgaps.cc:282) followed by exg_seq(0,0): `seq` is
   (len)*many residue codes [pos][member] for positions 0..len-1; the library adds the sentinel
   columns.  weight may be NULL. */
g2g_group *g2g_group_create(g2g_ctx *ctx, const g2g_params *prm, int many, int len,
                            const uint8_t *seq, const double *weight);
void       g2g_group_free(g2g_group *g);

/* <-> PwdM::PwdM(mSeq** seqs, const ALPRM*) (src/maln2.cc:254): selects alnmode, swaps so the
   profile side is `a`, builds thickness / vectors / gap profiles.  *swapped receives PwdM::swp. */
g2g_pwdm  *g2g_pwdm_create(g2g_ctx *ctx, const g2g_params *prm, g2g_group *a, g2g_group *b, int *swapped);
/* n PwdMs at once with the derived arrays of all their groups -- column thickness (mSeq::mkthick, src/mseq.cc:149-354), frequency /
   profile vectors (mSeq::convseq, src/mseq.cc:392-587) and static gap profiles (Gfq::Gfq / seq2gfq, src/gfreq.cc:134-312) -- built
   ON THE DEVICE in one go (csrc/g2g_build.hip): what a sweep over hundreds of divisions wants.  Same objects and, bit for bit, the
   same arrays as n calls of g2g_pwdm_create (tests/test_gpu_builders.py).  Groups with nil codes (tgapf < 1) are built on the
   host inside the same call.  swapped (n ints) may be NULL.  On failure nothing is handed out. */
int        g2g_pwdm_create_batch(g2g_ctx *ctx, const g2g_params *prm, int n, g2g_group *const *a, g2g_group *const *b, int *swapped, g2g_pwdm **out);
void       g2g_pwdm_free(g2g_pwdm *p);
const g2g_problem *g2g_pwdm_problem(const g2g_pwdm *p);

/* <-> SKL* align2(mSeq* seqs[], PwdM* pwdm, VTYPE* scr, Gsinfo*) (src/maln2.cc:1875): forward fill,
   traceback, stdskl, end check with the sh = -100 retry.  *skl is malloc'ed: skl[0..*nskl) corners
   ascending (the reference's skl[1..n]); caller g2g_free()s.  Batched form = one randiv sweep. */
/* ---- f1: the sum-of-pairs score of the alignment a skeleton describes ---------------------------------
 * <-> VTYPE PreSpScore::calcSpScore(Gsinfo*) (src/fspscore.cc:584-622) = SpScore<SPunit|SPunit_hf|SPunit_pf>::calcSkl
 * (src/fspscore.h:202-254, calscr src/fspscore.cc:346-541) followed by PwdM::rescale (src/maln2.cc:245-252): the score is
 * re-evaluated ALONG the path (column scores, unpaired-column penalties and the gap-open counts of the gap-profile
 * algebra) and returned per unit pair weight; Prrn::onecycle takes fstat.val of the old and the new alignment as the
 * acceptance delta.  On this path: NGP / HLF / RHF / GPF modes and the naive units SPunit_nv / _w11 / _w21 / _w22 of the
 * NTV modes, with Noll 2 and 3 (-yl3: the long-gap bookkeeping `Gep1st`, src/mseq.cc:658-758, included).  mch/mmc/unp of
 * FSTAT (PwdM::stt2) are not computed.                                                                             */
typedef struct {
    double vab;          /* PwdM::Vab = scale * wa * wb (src/maln2.cc:234)                         */
    double basic_gep;    /* PwdB::BasicGEP = -u * axbscale (src/aln2.cc:103)                       */
    double diffu;        /* PwdB::diffu = LongGEP - BasicGEP (src/aln2.cc:105)                      */
    double diff_u;       /* PwdM::diff_u = scale * (u - u1) (src/maln2.cc:233): weight of the long-gap count `lunp` in
                            PwdM::wgop (maln.h:321-325); only read when Noll = 3                                */
    int32_t flags;       /* G2G_SP_NOSTATS: leave FSTAT's mch / mmc / unp at 0 (the statistics cost about a third of the walk;
                            a refinement loop reads val and raw only)                                               */
    int32_t reserved;
} g2g_spparams;
#define G2G_SP_NOSTATS 1
typedef struct {
    double  val, gap;    /* FSTAT::val / gap after PwdM::rescale: per unit pair weight (what align2 leaves in Gsinfo.fstat)      */
    int32_t status, reserved;
    double  raw;         /* the score BEFORE rescale = the return value of PreSpScore::calcSpScore(SKL*), src/fspscore.cc:544-582:
                            Prrn::onecycle takes THIS for the current alignment and fstat.val for the new one (src/prrn5.cc:523,535) */
    double  mch, mmc, unp;   /* FSTAT::mch / mmc / unp after rescale: matched, mismatched and unpaired member pairs per unit pair
                                weight (PwdM::stt?? src/maln2.cc:627-850,1300-1450; the naive units count in calcstat)        */
} g2g_fstat;
/* level 0: on a prepared batch (inputs resident in HBM); skl[i] = the standardised skeleton of problem i
 * (g2g_stdskl output: corners ascending, first = (a.left, b.left), last = (a.right, b.right))              */
int        g2g_batch_spscore(g2g_batch *b, const g2g_spparams *sp, const g2g_skl *const *skl, const int *nskl,
                             g2g_fstat *out);
/* ... nsets skeletons per problem of the batch in one launch: entry e (of nsets * n) is set e / n of problem e % n */
int        g2g_batch_spscore_sets(g2g_batch *b, int nsets, const g2g_spparams *sp, const g2g_skl *const *skl, const int *nskl,
                                  g2g_fstat *out);
/* level 1 */
int        g2g_pwdm_spparams(const g2g_pwdm *p, g2g_spparams *sp);
int        g2g_spscore_batch(g2g_ctx *ctx, int n, g2g_pwdm *const *p, const g2g_skl *const *skl, const int *nskl,
                             g2g_fstat *out);
int        g2g_spscore_batch_flags(g2g_ctx *ctx, int n, g2g_pwdm *const *p, const g2g_skl *const *skl, const int *nskl,
                                   int flags, g2g_fstat *out);       /* the same with g2g_spparams::flags set for every item */
/* What a refinement needs of a window of divisions in one call: align2() of every pair (as g2g_align2_batch: scr, skl,
   nskl, status) plus calcSpScore of its CURRENT alignment `cur` (fs_cur) and of the new one (fs_new), flags as for
   g2g_spscore_batch_flags (<-> Prrn::onecycle, src/prrn5.cc:522-535).  Same results as the two calls; the problems are
   packed and uploaded once. */
int        g2g_align2_score_batch(g2g_ctx *ctx, int n, g2g_pwdm *const *pw, const g2g_skl *const *cur, const int *ncur, int flags,
                                  double *scr, g2g_skl **skl, int *nskl, int *status, g2g_fstat *fs_cur, g2g_fstat *fs_new);
int        g2g_align2(g2g_ctx *ctx, g2g_pwdm *p, double *scr, g2g_skl **skl, int *nskl);
/* <-> VTYPE HomScore(mSeq* seqs[], PwdM* pwdm, long rr[]) (src/maln2.cc:1837): score only; rr may be NULL. */
int        g2g_homscore(g2g_ctx *ctx, g2g_pwdm *p, double *scr, int64_t rr[2]);
int        g2g_align2_batch(g2g_ctx *ctx, int n, g2g_pwdm *const *p, double *scr,
                            g2g_skl **skl, int *nskl, int *status);

/* ---- f2: the refinement loop --------------------------------------------------------------------------------------
 * <-> Prrn::rir (reference src/prrn5.cc:633-666) with onecycle / divideseq / gather / calcfact (:414-543), Randiv in TREEDIV
 * mode + McRand (src/randiv.cc:34-239, the glibc rand() seeding included), delcommongap / synthgap (src/mgaps.cc:181-369) and
 * gap2skl (src/gaps.cc:274): randomised iterative refinement of an MSA over the branches of its weighting tree.  The SERIAL
 * trajectory of the reference is reproduced -- same branch sequence, same accepted moves, same final MSA -- while the DPs of a
 * WINDOW of upcoming divisions run as one batch on the GPU (speculation: the divisions behind an accepted move are drawn again).
 *   codes: len x many residue codes [column][member] (gap = 1), no all-gap column.
 *   tree : Ktree::lead[] (src/phyl.h): node id = tid, leaves 0 .. many-1 are the members, left / right / parent = -1 where
 *          absent, vol / cur = the Kirchhoff weights of Ktree::calcpw.  g2g_ktree_from_msa (below) builds it from the MSA
 *          itself -- the reference's tree, bit for bit; a tree from elsewhere is taken as it is.
 *   opts : seed (Randiv's rn: 1 = "seed from rand()" as prrn does), maxitr (prrn -I, default 10), window (largest speculative
 *          batch, default 32).  rank / world / exchange: with world > 1 every rank calls g2g_refine with the SAME inputs; a
 *          window is sharded (largest rectangles first, round-robin), each rank scores its share and `exchange` all-gathers
 *          the fixed-size result slots (n_ints int32 per rank in, world x n_ints out, rank-major) -- RCCL / MPI / gloo on the
 *          caller's side; every rank then takes the same decisions and ends with the same MSA.  Return 0 from the callback.
 * Outputs: *out_codes (malloc'ed, *out_len x many; g2g_free), the trajectory (*steps, malloc'ed; may be NULL) and counters. */
typedef struct g2g_tree {
    int32_t n_nodes;                /* 2 * many - 1                                                */
    const int32_t *left, *right, *parent;
    const double  *vol, *cur;
} g2g_tree;
typedef int (*g2g_exchange_fn)(void *user, const int32_t *mine, int n_ints, int32_t *all);
/* Optional: the caller scores the divisions of a window instead of the GPU (ctx may then be NULL).  For each of the n PwdMs:
   scr[i] = the DP score and skl[i] / nskl[i] = the standardised skeleton of align2() (malloc'ed, the library frees it),
   raw_cur[i] = calcSpScore(SKL*) of the CURRENT alignment cur[i] (not rescaled), val_new[i] = fstat.val of the new one.
   The tests drive the loop -- window logic, sharding, exchange, error paths -- on a machine without a GPU this way, with the
   CPU checker in the scorer's seat; the product never sets it.  Return 0. */
typedef int (*g2g_score_fn)(void *user, int n, g2g_pwdm *const *pw, const g2g_skl *const *cur, const int *ncur,
                            double *scr, g2g_skl **skl, int *nskl, double *raw_cur, double *val_new);
/* An accepted move: the two member lists of the division (larger group first, as Prrn::divideseq orders them) and the new
   skeleton in that order (corners over the two groups' columns with their all-gap columns dropped). */
typedef void (*g2g_accept_fn)(void *user, int branch, int na, const int32_t *la, int nb, const int32_t *lb, int nskl, const g2g_skl *skl);
typedef struct g2g_refine_opts {
    int32_t seed, maxitr, window;
    int32_t rank, world, slot_cap;  /* slot_cap: most corners of a skeleton an exchange slot holds (default 4096) */
    g2g_exchange_fn exchange;       /* A rank that fails locally still enters the exchange: its error code travels in the first
                                       word of its buffer and EVERY rank returns it after the gather (no rank is left waiting in
                                       the collective).  The callback itself must fail on all ranks or on none.                */
    void   *exchange_user;
    g2g_score_fn scorer;            /* NULL: g2g_align2_batch + g2g_spscore_batch on the GPU                                   */
    void   *scorer_user;
    g2g_accept_fn on_accept;        /* optional: told about every accepted move, in order (what synthgap applies, src/prrn5.cc:536-541) */
    void   *on_accept_user;
    int32_t window_min, reserved;   /* window after an accepted move (default: 16 when len x len >= 2^22 -- MSAs of 2048 columns or more --, else 4); it doubles up
                                       to `window` while nothing is accepted */
} g2g_refine_opts;
typedef struct g2g_refine_step {
    int32_t branch, na, nb, swp, accepted, skipped;   /* skipped: neither group had a column to drop -- no DP (prrn5.cc:497) */
    double  scr, val_new, val_old, delta;             /* DP score; fstat.val of the new alignment; raw score of the current one */
    double  t_ms;                                     /* wall clock since the call began when this division's window had been scored */
} g2g_refine_step;
typedef struct g2g_refine_stats {
    int32_t divisions, accepted, batches, divisions_scored_here, divisions_wasted;
    int32_t wait_timeouts, recovered_dps, reserved;   /* scheduler waits that ran into their limit during the call / DPs re-run (g2g_ctx_counters) */
} g2g_refine_stats;
int        g2g_refine(g2g_ctx *ctx, const g2g_params *prm, int many, int len, const uint8_t *codes, const g2g_tree *tree,
                      const g2g_refine_opts *opts, uint8_t **out_codes, int *out_len, g2g_refine_step **steps, int *nsteps,
                      g2g_refine_stats *stats);

/* ---- the weighting tree of an MSA ----------------------------------------------------------------------------------
 * <-> Ssrel::calcweight (reference src/prrn5.cc:385-386): Ktree(msd) -- calcdistseq / pairdvn (src/phyl.cc:344-385,
 * src/divseq.cc:33-63: the divergence of every pair of members over the columns of the alignment), DistTree::upg_method
 * (src/phyl.cc:911-1026, UPGMA) and Knode::teachparent (:583-595) -- followed by Ktree::calcpw -> pairwt (:704-767, 813-826: the
 * Kirchhoff weights vol / cur).  The divergences are computed on the GPU (csrc/g2g_ktree.hip: one launch for all pairs), the
 * tree and the weights on the host; topology, heights and weights are the reference's, bit for bit.
 *   codes  : len x many residue codes [column][member] as for g2g_refine; a code <= 1 is a gap (nil 0 counts as one: IsGap).
 *   dist   : many (many - 1) / 2 doubles, pair (i < j) at j (j - 1) / 2 + i (the reference's elem()): 1 - mch / (0.8 gap + 0.2 unp +
 *            mch + mmc) in the reference's operation order; a pair without any column gives what IEEE gives (NaN).
 *   counts : 4 int32 per pair (matched, mismatched, unpaired columns, gaps opened), same order; may be NULL.
 * Limits: 2 <= many <= 4096, len >= 1 (else G2G_ERR_ARG).  (Entry points added without a change of g2g_abi_version.) */
typedef struct g2g_ktree {          /* all arrays malloc'ed, n_nodes = 2 * many - 1 long; release with g2g_ktree_free              */
    int32_t n_nodes, root;          /* root: the node made last (n_nodes - 1)                                                    */
    int32_t *left, *right, *parent, *ndesc;   /* -1 where absent; ndesc = leaves below the node (1 for a leaf)                   */
    double  *height, *length, *res, *vol, *cur;   /* Knode::height (half the merge distance), ::length (branch to the parent),
                                       ::res (resistance of the subtree), and the Kirchhoff weights                             */
} g2g_ktree;
int        g2g_msa_divergence(g2g_ctx *ctx, int many, int len, const uint8_t *codes, double *dist, int32_t *counts);
/* The tree of a distance matrix in that layout: host only, needs no context; dist is not modified.  with_weights = 0 is the
   Ktree(&dm) of the progressive start (src/prrn5.cc:978-979): topology, heights, lengths and res only, vol / cur are zero.
   A NaN or negative distance: G2G_ERR_ARG, g2g_last_error names the pair.  left / right / parent / vol / cur are directly
   usable as a g2g_tree. */
int        g2g_ktree_from_dist(int many, const double *dist, int with_weights, g2g_ktree *out);
/* = g2g_msa_divergence + g2g_ktree_from_dist(with_weights = 1) */
int        g2g_ktree_from_msa(g2g_ctx *ctx, int many, int len, const uint8_t *codes, g2g_ktree *out);
void       g2g_ktree_free(g2g_ktree *t);

/* <-> VTYPE Ssrel::pairsum_ss(mSeq* sd, bool use_pw) (reference src/fspscore.cc:896-922; Sptree::sptree :784-821): the weighted
 * sum-of-pairs score of a whole MSA, the number prrn reports for an alignment (initial / refined, the -O4 line).  The reference
 * walks the weighting tree: a node of at most ndesc_thr = 60 leaves is scored naively (Msap::ps_nml with the pair weights of
 * Ktree::recalcpw when use_pw), a larger node is the sum of its children plus the score BETWEEN their two groups
 * (calcscore_grp: PwdM + SpScore::calcJxt).  Here the naive nodes run on the GPU (g2g_pairsum_kernel) and the joins through the
 * level-1 builders + g2g_batch_spscore; the sum is formed in the reference's order.  codes / tree as for g2g_refine.
 * Not on this path: tgapf != 1, the ether term (u0), exon-boundary annotations (spSigII), subset trees (ss->num < ss->elms). */
int        g2g_pairsum(g2g_ctx *ctx, const g2g_params *prm, int many, int len, const uint8_t *codes, const g2g_tree *tree,
                       int use_pw, double *out);

/* ---- f3: the guide-tree stage -- score-only pairwise DPs between single sequences ----------------------
 * <-> VTYPE alnScoreD(const Seq* seqs[], const Simmtx* sm, int* ends = 0) (reference src/fwd2d1.cc:324-338), global branch:
 * Fwd2d::Fwd2d (the boundary values, :58-93), Fwd2d::forwardD (:136-158, anti-diagonal order, affine gaps -(v + k u),
 * band = stripe(seqs, alprm.sh), src/aln2.cc:156-174) and Fwd2d::lastD (:100-134, terminal-gap discount tgapf).  This is what
 * dpscore() (src/phyl.cc:222-252) runs for every pair of members when the distance matrix comes from alignment scores.
 * Sequences are uploaded once, pairs are index pairs; scores are bit-equal to the reference's doubles.
 * prm: u, v, scale (floats in the reference: the library forms (float) u * (float) scale as the reference does), tgapf, sh,
 * simmtx / simdim / simrows (Simmtx::mtx as doubles).  Not on this path: the local (algmode.lcl) and `ends` variants.  */
typedef struct g2g_dseq {
    const uint8_t *res;             /* Seq::at(0): len residue codes (one member)                 */
    int32_t len, left, right;       /* Seq::len, ::left, ::right                                  */
} g2g_dseq;
int        g2g_alnscored_batch(g2g_ctx *ctx, const g2g_params *prm, int nseq, const g2g_dseq *seqs,
                               int npairs, const int32_t *ia, const int32_t *ib, double *score, int32_t *status);
/* <-> SKL* alignB_ng(const Seq* seqs[], const PwdB* pwd, VTYPE* scr) (reference src/fwd2b1.cc:1347-1353 -> globalB_ng :1286-1315
 * -> lspB_ng :1053-1095).  DPs of fewer than MaxVmfSpace cells (16 Mi; context option MAX_VMF_SPACE <-> setVmfSpace, vmf.cc:27) are
 * traced in one piece (trcbkalignB_ng :1025-1051): Aln2b1::forwardB_ng (:145-279; affine gaps, with prm->ls = 3 the second,
 * long-gap pair of layers) + initB_ng / lastB_ng (:64-143) + the Vmf record chain.  Larger ones go through the reference's
 * linear-space recursion: centerB_ng (:492-782, with binitB_ng / finitB_ng :382-490) splits the DP at the middle row into two
 * parts with narrowed windows, the parts recurse (a part of one diagonal: diagonalB_ng's two records, :1015-1021), the value is
 * the top centre's.  Then stdskl.  PwdB's constants (BasicGOP ... codonk1, src/aln2.cc:80-120) are formed from prm's u, v, u1, k1,
 * ls, scale, molc as the reference does.  skl[i]: malloc'ed corners ascending (g2g_free), nskl[i] of them.
 * Status G2G_ERR_MODE: a band of one diagonal at the top level; sides of 46341 and more (the reference's int volume overflows);
 * a pair on which centerB_ng hands back a part that is no DP (seen with ls = 3: the reference itself reads outside its arrays and
 * crashes there).  Local modes are not on this path. */
int        g2g_alignb_ng_batch(g2g_ctx *ctx, const g2g_params *prm, int nseq, const g2g_dseq *seqs, int npairs,
                               const int32_t *ia, const int32_t *ib, double *scr, g2g_skl **skl, int *nskl, int32_t *status);

/* ---- k-mer composition distances between unaligned single sequences ---------------------------------------------------
 * <-> FTYPE* calcdist_kmer(Seq** seqs, int nn, int inm, Strlist*& snm) (reference src/qdiv.cc:245-282), the distance matrix
 * DistMat(Seq**, nn) holds (src/phyl.cc:515-528) when makemsa runs with algmode.any == Composition (src/prrn5.cc:976-979), and
 * AdjacentMat::dist_kmer per candidate pair (src/adjmat.cc:90-97): the cheap guide-tree distance, no DP.
 *   words : Kcomp::makeHash (qdiv.cc:61-80) with the continuous seed (Bitpat_wq::word / flaw, src/bitpat.cc:168-185).  The scan reads
 *           the residues left .. right - k - 1 and counts a word wherever the last k residues read were all elementary (the 20
 *           amino acids, or A C G T): an ungapped sequence of elementary residues has max(0, (right - left) - 2 k + 1) words.
 *           Any other residue (X, B, Z, N and the other ambiguity codes, gap, nil) breaks the word -- the reference reads table
 *           entries it never wrote for them (bitpat.cc:76-86); here no word that contains one is counted.
 *   pair  : qdiv (qdiv.cc:179-232, many == 1): s = the sum over shared words of the smaller count, f = s / min(Ta, Tb) with
 *           Ta, Tb the word totals, d = 1 - f; then by DistMes (src/aln.h:54)
 *             0 QFdiv d   1 QFidn f   6 NJuCa jukcan(d)
 *           and, after f = 0.18704 * log((0.00501 + f) / (0.00501 + 1.)) + 1., d = 1. - f,
 *             2 QCdiv d   3 QCidn f   4 QJuCa jukcanpro(d)   5 Qpamd pamcorrect(d) / 100. (corr_mhits == 0)
 *           (jukcan / jukcanpro / pamcorrect: src/divseq.cc:107-139; out of range gives OUTOFRANGE = 1024).  The stored distance
 *           is 100 * qdiv (kcmp_main, qdiv.cc:239).  A member without any word gives 0 / 0 = NaN with every partner, as in the
 *           reference.  Defaults (qdiv.cc:32-33): protein k = 5 with Qpamd, DNA k = 10 with QJuCa (DNA does go through jukcanpro).
 * The parameters are taken literally: resetqdiv's swapping of one molecule's defaults for the other's (qdiv.cc:45-57) is not
 * reproduced.  The device (csrc/g2g_kmer.hip) sorts and counts the words and intersects the lists -- integers only: s, Ta, Tb per
 * pair; the doubles are formed on the host in the reference's operation order.  Nothing is sorted on the host.
 * Limits (else G2G_ERR_ARG): k 1 .. 6 for protein, 1 .. 15 for DNA (beyond them the reference's 32-bit (queue * nalpha + c) % TabSize,
 * bitpat.cc:183, no longer forms the true words); measure -1 .. 6; reserved 0; 2 <= nseq, and nseq <= 4096 in the all-pairs form;
 * at most 16384 word positions ((right - left) - 2 k + 1) per sequence -- g2g_last_error names the sequence; 0 <= left <= right <= len.
 * Not on this entry: reduced alphabets and spaced seeds -- g2g_kmer_dist_batch_spec below has them.  On neither: profiles of
 * groups (many > 1), reading frames, corr_mhits != 0.
 * (Entry points added without a change of g2g_abi_version.) */
typedef struct g2g_kmer_params {
    int32_t molc;      /* 1 PROTEIN, 2 DNA */
    int32_t k;         /* 0: the reference's default (5 / 10) */
    int32_t measure;   /* DistMes value 0..6; -1: the default (Qpamd / QJuCa) */
    int32_t reserved;
} g2g_kmer_params;
/* dist[p] = 100 * qdiv(a, b); counts (may be NULL): s, Ta, Tb per pair.
   ia == ib == NULL: all pairs, pair (i < j) at j (j - 1) / 2 + i, npairs = nseq (nseq - 1) / 2.
   A pair (i, i) is legal.  Arguments are checked before the device is asked for. */
int        g2g_kmer_dist_batch(g2g_ctx *ctx, const g2g_kmer_params *kp, int nseq, const g2g_dseq *seqs,
                               int npairs, const int32_t *ia, const int32_t *ib, double *dist, int32_t *counts);
/* host only, no context: the closed form from the three integers of each pair */
int        g2g_kmer_dist_from_counts(const g2g_kmer_params *kp, int npairs, const int32_t *counts, double *dist);

/* ---- the same with a residue classification and a seed: all three inputs of setqdiv(k, ap, bp, dm) (qdiv.cc:36-43) -------
 *   classes : classes[code] is the class of a residue code (what ReducWord builds from a pattern such as A|C|D|EQ|FY|...,
 *             src/bitpat.cc:59-95; the caller supplies the table, none is built in).  A class >= nalpha -- 0xFF is one -- and a
 *             code >= nclasses break a word at the positions the seed examines.  Words are base-nalpha numbers of classes.
 *   seed    : NULL: the continuous seed of k, as above with base nalpha -- (right - left) - 2 k + 1 word positions.  Else a string
 *             of '1' / '0' (Bitpat::Bitpat, Bitpat_wq::word / flaw, bitpat.cc:99-131, 168-202), width = its length, weight = its
 *             number of '1's: the scan reads the residues left .. right - width - 1; after residue p >= left + width - 1 the word is
 *             formed of the classes at p - width + 1 + o for the offsets o of the '1's, left to right, and counted iff each of them is
 *             < nalpha (a bad residue under a '0' breaks nothing): (right - left) - 2 width + 1 word positions.  An all-ones seed gives
 *             the continuous result.
 *   pair    : as above, with the row of qdiv's param (qdiv.cc:181-186, 214-222) chosen by nalpha as given and by k, also where a seed
 *             string is given: nalpha 14 with k 3 / 4 / 5 -> (0.92042, 0.18677) / (0.34576, 0.07108) / (0.22333, 0.03164), every other
 *             case (0.18704, 0.00501).
 * Limits (else G2G_ERR_ARG, before the device is asked for): nalpha 0 (= 20 / 4) or 2 .. 20 (protein) / 2 .. 4 (DNA), and the full
 * alphabet where classes is NULL; nclasses 1 .. 256; k 1 .. 15 (0: the default, 5 / 10); without a seed string
 * nalpha^(k + 1) <= 2^32 (beyond it the reference's 32-bit queue no longer holds the true words); a seed string of '0' / '1' only,
 * first and last character '1', width <= 32, weight 1 .. 15, nalpha^weight < 2^32; reserved 0; at most 16384 word positions per
 * sequence, counted with the width; the rest as for g2g_kmer_dist_batch.  Not on this path: groups (many > 1), reading frames,
 * corr_mhits != 0, and the reference's own alphabet tables (for protein with Nalpha 6 .. 20 it ignores a caller's pattern).
 * With nalpha 0, classes NULL and seed NULL both functions return what g2g_kmer_dist_batch / g2g_kmer_dist_from_counts return. */
typedef struct g2g_kmer_spec {
    int32_t molc, k, measure, nalpha;   /* k 0 / measure -1 / nalpha 0: the defaults */
    const uint8_t *classes;             /* classes[code], code < nclasses; NULL: the full alphabet of g2g_kmer_dist_batch */
    int32_t nclasses, reserved;         /* reserved 0 */
    const char *seed;                   /* NULL: continuous seed of k */
} g2g_kmer_spec;
int        g2g_kmer_dist_batch_spec(g2g_ctx *ctx, const g2g_kmer_spec *sp, int nseq, const g2g_dseq *seqs,
                                    int npairs, const int32_t *ia, const int32_t *ib, double *dist, int32_t *counts);
/* host only, no context; classes and nclasses are not looked at */
int        g2g_kmer_dist_from_counts_spec(const g2g_kmer_spec *sp, int npairs, const int32_t *counts, double *dist);

/* ---- the conserved regions of an MSA ---------------------------------------------------------------------------------
 * <-> Ssrel::consreg / Ssrel::constwo (reference src/consreg.cc:438-518), the first step of prrn's default refinement
 * (IterMsa::preprrn, src/prrn5.cc:785-839): the MSA is cut at every branch of its weighting tree into two sons that keep the
 * father's columns; per division a PwdM and one walk over the columns -- s = sim2 of the column plus the gap term of a diagonal
 * step, cons2_ng / _nv / _hf / _pf (consreg.cc:170-406) by the PwdM's banded mode -- and a thresholded running sum over s gives
 * ranges of columns; the ranges of all divisions are intersected (cmnrng, src/css.cc:261-282).  The column scores and the scan
 * run on the GPU (csrc/g2g_consreg.hip: one workgroup per division), in the reference's order of double additions.
 * Not on this path: Conserved1, findoutliers (refinement restricted to ranges: g2g_refine_plan and g2g_refine_planned below).
 * (Entry points added without a change of g2g_abi_version.) */
typedef struct { int32_t left, right; } g2g_range;

/* <-> Ssrel::constwo on n built pairs whose two groups have the SAME length (juxtaposed sons of one MSA).
   thr: ALPRM::thr.  ranges[i] malloc'ed (g2g_free), nranges[i] entries, ascending, columns of the groups.
   colscore may be NULL; else colscore[i] receives len_i doubles, the s of every column (malloc'ed).
   status (n ints) may be NULL.  G2G_ERR_MODE: a pair in a mode that is not banded, annotated groups, groups with discounted
   terminal gaps; G2G_ERR_ARG: groups of unequal length or not standing whole (left = 0, right = len), thr <= 0.  A pair that
   cannot be served fails the call, g2g_last_error names it.  Arguments are checked before the device is asked for.           */
int g2g_constwo_batch(g2g_ctx *ctx, int n, g2g_pwdm *const *pw, double thr,
                      g2g_range **ranges, int *nranges, double **colscore, int *status);

/* <-> Ssrel::consreg(msd, dissim): all 2 many - 3 branches of `tree`, sons extracted with every column kept,
   weight (many doubles, may be NULL) handed down as Seq::extseq does; the intersection of the divisions'
   ranges, or with dissim its complement in [0, len).  prm is the caller's localprm (u, v, scale, ls, k1,
   tgapf, simmtx = the matrix the reference would use: number 1); prm->banded must be 1.
   The reference's localprm (consreg.cc:39-40): u 3, v 10, u0 0, u1 0, tgapf 1, scale 1, k1 7, ls 2, sh 100, thr 35.
   *out malloc'ed (g2g_free; an empty result is a valid pointer with *nout = 0).
   G2G_ERR_MODE: banded != 1, u0 > 0, tgapf != 1; G2G_ERR_ARG: many < 3, thr <= 0, a malformed tree.                          */
int g2g_consreg(g2g_ctx *ctx, const g2g_params *prm, double thr, int many, int len, const uint8_t *codes,
                const double *weight, const g2g_tree *tree, int dissim, g2g_range **out, int *nout);

/* host only, no context: what g2g_consreg finishes with, on plain ascending lists of disjoint ranges.  dissim = 0: cmnrng(a, b, 0),
   the intersection with empty pieces dropped (len is not read); dissim = 1: complerng, [0, len) without the ranges of a (b is not
   read).  *out malloc'ed (g2g_free). */
int g2g_ranges_combine(const g2g_range *a, int na, const g2g_range *b, int nb, int dissim, int len, g2g_range **out, int *nout);

/* ---- fused groups and the per-range refinement plan -------------------------------------------------------------------
 * <-> ConservedT::mayfuse / testssrel / rearrange, Ssrel::consregss, Ssrel::consreg over a relation with groups (reference
 * src/consreg.cc:452-464, 569-589, 667-711, 484-518) and what IterMsa::preprrn decides with them (src/prrn5.cc:794-823): subtrees
 * of the weighting tree whose two sons are conserved from end to end are fused into groups, the unconserved column ranges are
 * sought over the grouped relation, and inside every range the groups are fused again.  The fuse test walks the column scores
 * of g2g_constwo_batch with another recurrence (scr += s; a positive scr becomes 0; the walk breaks where scr < fthr) on the GPU
 * (g2g_mayfuse_kernel in csrc/g2g_consreg.hip: one workgroup per test).
 * The plan is run by g2g_refine_planned below.  Not on this path: recalcpw of a fused tree, Conserved1, findoutliers.
 * (Entry points added without a change of g2g_abi_version.) */
typedef struct g2g_subset {         /* Subset (src/sets.h:27-31): group g holds member[start[g] .. start[g + 1])                  */
    int32_t num, elms;              /* groups; members in all                                                                    */
    int32_t *start, *member;        /* num + 1 and elms ints; malloc'ed when the library hands a subset out (g2g_subset_free)    */
} g2g_subset;
void g2g_subset_free(g2g_subset *s);
typedef struct g2g_relation {       /* a subset and the tree over its groups (Ssrel: ss + ktree); release with g2g_relation_free  */
    int32_t fused;                  /* 0: nothing fused -- the reference's NULL; the relation repeats the one that was given     */
    g2g_subset ss;
    int32_t n_nodes;                /* 2 * ss.num - 1: leaf g is group g, the other nodes in post-order, the root last           */
    int32_t *left, *right, *parent; /* -1 where absent                                                                           */
    int32_t *origin;                /* the node of the given tree each node was copied from (Knode fields are copies: vol, cur)  */
    double  *vol, *cur;
} g2g_relation;
void g2g_relation_free(g2g_relation *r);
typedef struct g2g_fuse_stats { int32_t tests, fused, launches, reserved; } g2g_fuse_stats;

/* <-> ConservedT::mayfuse on n built pairs whose two groups are juxtaposed sons of equal length.  u, v: ALPRM::u, ::v (floats in
   the reference; fthr = (VTYPE) -((2 u + v)) * a->sumwt * b->sumwt, consreg.cc:73).  fuse[i] 1: the walk reached the last column;
   stop_col[i]: the column at which scr < fthr first held, -1 when fused.  Refusals as g2g_constwo_batch, all before the device
   is asked for; a NULL context with good arguments is G2G_ERR_ARG.                                                              */
int g2g_mayfuse_batch(g2g_ctx *ctx, int n, g2g_pwdm *const *pw, double u, double v, int *fuse, int *stop_col, int *status);

/* <-> Ssrel::consregss on the columns [left, right) of an MSA (what restrange + consregss computes).  tree: the relation's tree,
   its leaves 0 .. k - 1 are the relation's groups (groups NULL: the members themselves, k = many).  The tests run level by level:
   round r holds the inner nodes whose two sons are leaves or were fused in earlier rounds -- the tests of the reference's post-
   order walk, none else -- and is one g2g_mayfuse_batch on sons built by the level-1 builders.  Groups are numbered in leaf
   post-order, left before right; a fused node hands its members over from left to right.  Everything fused: one group, a tree
   of one node.  G2G_ERR_MODE: banded != 1, u0 > 0, tgapf != 1; G2G_ERR_ARG: a malformed tree or subset, an empty or out-of-bounds
   range, many < 2.  stats may be NULL.                                                                                          */
int g2g_consregss(g2g_ctx *ctx, const g2g_params *prm, int many, int len, const uint8_t *codes, const double *weight,
                  const g2g_tree *tree, const g2g_subset *groups, int left, int right, g2g_relation *out, g2g_fuse_stats *stats);

/* <-> Ssrel::consreg over a relation with groups: the 2 num - 3 divisions of the tree over the groups in Randiv's numbering
   (num = 2: the one division), member lists expanded through the groups (bin2lst2g, src/randiv.cc:88-100).  groups NULL:
   g2g_consreg (but two members are served).                                                                                     */
int g2g_consreg_groups(g2g_ctx *ctx, const g2g_params *prm, double thr, int many, int len, const uint8_t *codes,
                       const double *weight, const g2g_tree *tree, const g2g_subset *groups, int dissim, g2g_range **out, int *nout);

/* What preprrn decides before any Prrn is built, from the unrefined MSA and its weighting tree (g2g_ktree_from_msa): the whole-MSA
   relation (consregss), the attack ranges (consreg(DISSIM) over it, ascending), and per range its own relation (consregss inside
   the range, over the whole-MSA relation; origin names nodes of `whole`) and whether it touches column 0 / len -- where exgl /
   exgr are kept (prrn5.cc:814-815).  The ranges' fuse rounds share launches.  status G2G_PLAN_NOTHING_TO_REFINE: the whole-MSA
   relation has fewer than two groups; there are no ranges then.  Release with g2g_refine_plan_free.                             */
#define G2G_PLAN_OK 0
#define G2G_PLAN_NOTHING_TO_REFINE 1
typedef struct g2g_refine_plan_t {
    int32_t status, nranges;
    g2g_relation whole;
    g2g_range *ranges;
    int32_t *at_left, *at_right;
    g2g_relation *range_rel;
    g2g_fuse_stats stats;           /* over the whole call; launches: g2g_mayfuse_batch calls                                   */
} g2g_refine_plan_t;
int  g2g_refine_plan(g2g_ctx *ctx, const g2g_params *prm, double thr, int many, int len, const uint8_t *codes,
                     const double *weight, const g2g_tree *tree, g2g_refine_plan_t *out);
void g2g_refine_plan_free(g2g_refine_plan_t *p);

/* ---- g2g_refine over the plan: prrn's default refinement (local_thr = 35) ------------------------------------------------
 * <-> the loop of IterMsa::preprrn over the attack ranges (reference src/prrn5.cc:806-818): one Prrn (:688-781) per range, from
 * the LAST range to the first, on the columns [left, right) of the current MSA and over plan->range_rel[r] (url = trl ? trl :
 * srl).  A range's result replaces its columns and may be longer or shorter; the ranges still to come lie to its left, so their
 * coordinates stay valid.  A range whose relation has fewer than two groups is skipped and draws nothing (Prrn::Prrn, num <= 1).
 * Per range the loop is g2g_refine's (the two entry points share it) with groups for leaves: cycle = 2 num - 3 (two groups: the one
 * division, once), a division's sides are the member lists expanded through the subset, each group in its own member order
 * (bin2lst2g, src/randiv.cc:88-100), larger side first by member count (totalNoSeq).  In the matrix form a fused group is a set
 * of columns of the matrix that always travel together.
 *   prm    : the parameters of the DPs (the reference's alnprm).
 *   plan   : NULL: the call makes it with g2g_refine_plan(ctx, prm, thr, ...) -- with the DPs' parameters (needs a context).  The
 *            reference decides its plan with parameters of its own (localprm and similarity matrix number 1, see g2g_consreg):
 *            a caller after the reference's run makes the plan with those and passes it.  Given, it is taken as it is (thr
 *            is not read) after validation -- every subset partitions the members, every tree has 2 num - 1 nodes and is checked
 *            as g2g_refine checks its tree, the ranges ascend, are disjoint and lie inside [0, len), origin is in range: else
 *            G2G_ERR_ARG.  With a plan and opts->scorer, ctx may be NULL.  G2G_PLAN_NOTHING_TO_REFINE, or no ranges: the input
 *            comes back unchanged with zero steps, G2G_OK.
 *   weight : msd->weight as phyl_pwt leaves it (many doubles; for the tree of g2g_ktree_from_msa: vol of the leaves), as for
 *            g2g_refine_plan.  A member of a fused group enters a builder as Ssrel::takeapart -> Seq::extseq(.., the group's vol)
 *            (src/consreg.cc:598-625) and Prrn::gather / aggregate leave it: weight[m] / vol[group], times what calcfact gives the
 *            group where the side holds several groups; a single member 1, times the same.  NULL: an MSA without weights -- a
 *            side made of one fused group has none, members of a side of several groups carry calcfact's factor alone.
 *   seed   : McRand (src/randiv.cc:34-53) draws rand() when the seed is 1 and then calls srand() on it: the second Prrn of a run
 *            starts from the rand() state the first one left.  One restated glibc generator serves the whole call.
 *   opts   : as for g2g_refine; maxitr, window, window_min (its default by the RANGE's length), scorer, on_accept (member lists,
 *            expanded) and exchange / world > 1 apply per range.
 *   steps  : the ranges' steps one after the other in processing order (last range first); branch is a node of that range's
 *            relation tree.  rstat: one entry per range of the plan in the plan's order, skipped ranges with nsteps = 0 (g2g_free;
 *            both may be NULL).  stats sums over the ranges.
 * G2G_ERR_MODE: tgapf != 1, u0 > 0, banded != 1 (as the plan; with tgapf = 1 the exgl / exgr switch of prrn5.cc:814-815 changes
 * nothing the DP reads: at_left / at_right are carried into rstat and otherwise unused); a leaf group without any residue inside
 * its range (g2g_last_error names the range and the group).  All refusals come before any scoring.
 * Not on this path: recycle > 1 (the caller builds a new tree and calls again); initsp / pairsum_ss over a relation with subsets
 * and recalcpw of a fused tree (the trajectory reads neither; gain is the difference the reference prints); best_of_n,
 * Conserved1, findoutliers.  (Entry point added without a change of g2g_abi_version.) */
typedef struct g2g_refine_range_stat {
    int32_t range, left, right;        /* index into plan->ranges; the columns before refinement */
    int32_t groups, cycle;
    int32_t first_step, nsteps;        /* slice of steps[] */
    int32_t divisions, accepted;       /* divisions = the reference's countaln of this Prrn */
    int32_t out_left, out_right;       /* the range's columns in the MSA as it stood when the range was done */
    int32_t at_left, at_right, reserved;
    double  gain;                      /* sum of the accepted deltas = sps - initsp of this Prrn */
} g2g_refine_range_stat;
int g2g_refine_planned(g2g_ctx *ctx, const g2g_params *prm, double thr, int many, int len, const uint8_t *codes,
                       const double *weight, const g2g_tree *tree, const g2g_refine_plan_t *plan,
                       const g2g_refine_opts *opts, uint8_t **out_codes, int *out_len,
                       g2g_refine_step **steps, int *nsteps, g2g_refine_range_stat **rstat, int *nrstat,
                       g2g_refine_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* G2G_H_ */
