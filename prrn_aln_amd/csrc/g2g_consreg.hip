// g2g_consreg.hip -- the conserved regions of an MSA: Ssrel::consreg / Ssrel::constwo (reference src/consreg.cc:438-518).
// The reference cuts the MSA at every branch of its weighting tree into two sons that keep the father's columns, builds a PwdM
// for the pair and walks the columns once: per column a group-to-group similarity plus the gap term of a diagonal step
// (cons2_ng / _nv / _hf / _pf, consreg.cc:170-406), a thresholded running sum over the column scores gives ranges, and the
// ranges of all divisions are intersected (cmnrng, src/css.cc:261-282).
// The column scores have one scorer on the device, cr_begin / cr_tile: one workgroup per pair of groups, lanes across the columns
// of a tile of CR_T columns.
//     1. members whose gap run in front of the column is read (_hf: b's, _nv: both sides'): one ballot per member and wave says
//        which of the tile's columns hold a residue; the run length of (member, column) is the distance to the nearest set bit
//        below the column -- in the lane's own wave, the waves in front of it, or the column carried in from earlier tiles
//        (Seq::pregap with left = 0 followed by incrgap, src/seq.cc:1870-1883, src/mgaps.cc:431-440).
//     2. a lane forms s of its column with the scorers of g2g_kernels.hip (sim2, crg2, newgap4) and stores it to LDS.
//     3. the kernel's lane 0 runs a recurrence of the reference over the tile's scores in column order; its scalars stay in
//        registers from tile to tile.
// The two kernels are their recurrences: g2g_consreg_kernel the thresholded running sum, whose ranges go to the division's slot in
// HBM, g2g_mayfuse_kernel the walk of the fuse test, which may leave early.  On the host both entries check a pair with
// cr_check_pair and reach the device through CrPairs.
// Plain launch on the context's stream; no atomics, no waits on other workgroups.
#include <hip/hip_runtime.h>

#define CR_T 256                      /* columns per tile = threads per workgroup */
#define CR_W (CR_T / 64)              /* waves */
#define CR_NV_MEM 8                   /* members of an _nv division (2 nj + ni < thr_gfq_21 = 8 allows four) */

struct ConsregArgs {
    double vthr;                      // PwdM::Vthr = Vab * thr (src/maln2.cc:235)
    int2 *ranges; int cap;            // the division's slot
    int *nranges;                     // ranges found (may exceed cap: the host reports it)
    double *colscore;                 // len doubles, or NULL
};

// run length of member j in front of column c (absolute), from the tile's residue masks and the carried column
__device__ __forceinline__ int cr_runlen(const unsigned long long *mask, const int *last, const int j, const int c0, const int c, const int wave, const int lane)
{
    unsigned long long m = mask[j * CR_W + wave] & ((1ull << lane) - 1ull);
    int w = wave;
    while (!m && w > 0) { --w; m = mask[j * CR_W + w]; }
    const int lastp1 = m ? c0 + w * 64 + (63 - __clzll((long long) m)) + 1 : last[j];
    return c - lastp1;
}

// PwdM::newgap2(asi, bs, glb), src/maln2.cc:850-879 (the _hf form of consreg only: the DP's newgap2 has dynamic lists)
__device__ double cr_newgap2(const DevProb &P, const int c, const unsigned long long *mask, const int *last, const int c0, const int wave, const int lane)
{
    double g = 0;
    const uint8_t *bs = res_at(P.b, c);
    const double *wt = P.b.weight;
    const SList adf = gfq_at(P.a, 1, c), acf = gfq_at(P.a, 0, c);
    for (int j = 0; j < P.b.many; ++j) {
        const double w = wt ? wt[j] : 1;
        const int glb = cr_runlen(mask, last, j, c0, c, wave, lane);
        if (bs[j] > 1) {
            for (int k = 0; adf.glen[k] >= 0; ++k) {
                if (glb < adf.glen[k]) break;
                g += adf.freq[k] * w;
            }
        } else {
            const double bu = 1;                               // mSeq::gapdensity of a gap without terminal discount (mseq.h:148-153)
            for (int k = 0; acf.glen[k] >= 0; ++k) {
                if (acf.glen[k] >= glb) g += acf.freq[k] * w * bu;
                else break;
            }
        }
    }
    return P.weighted_gop * g;
}

// ---- the tile scorer both kernels run ------------------------------------------------------------------------------------------
// a kernel's static LDS: arrays each kernel declares for itself, as before there was one scorer
struct CrShared {
    double *sc;                                                // [CR_T]: s of the tile's columns
    int *gl;                                                   // [CR_NV_MEM * CR_T], _nv: run lengths, [member][lane]
    int2 *zero_delta;                                          // [2], ZeroDelta: newgap4 over it is newgap(cf, df), src/gfreq.cc:493-505
    DevProb &P;
};
struct CrTiles {                                               // what a thread knows about its division once cr_begin has run
    int len, kind, an, nm;                                     // nm: members whose gap runs are read
    unsigned long long *mask;                                  // dynamic LDS [nm][CR_W]: the tile's columns with a residue, per member and wave
    int *last;                                                 // dynamic LDS [nm]: column behind the member's last residue in front of the tile
};

// The descriptor into LDS (one barrier), last[] and ZeroDelta set.  The caller sets what else it keeps in LDS and places the barrier
// that ends the prologue.
__device__ __forceinline__ CrTiles cr_begin(const CrShared &S, unsigned char *dyn, const DevProb *prob)
{
    const int tid = threadIdx.x;
    for (int i = tid; i < (int) (sizeof(DevProb) / 4); i += CR_T) ((int *) &S.P)[i] = ((const int *) prob)[i];
    __syncthreads();
    CrTiles T;
    T.len = S.P.a.right; T.kind = S.P.kind; T.an = S.P.a.many;
    T.nm = T.kind == 3 ? T.an + S.P.b.many : T.kind == 1 ? S.P.b.many : 0;
    T.mask = (unsigned long long *) dyn;
    T.last = (int *) (T.mask + (size_t) T.nm * CR_W);
    for (int j = tid; j < T.nm; j += CR_T) T.last[j] = 0;
    if (tid == 0) { S.zero_delta[0] = make_int2(0, 0); S.zero_delta[1] = make_int2(INT_MAX, 0); }
    return T;
}

// The tile that starts at column c0: the ballots, a barrier, s of every live column into S.sc (and into colscore where it is given),
// a barrier, last[] carried on to the next tile.  The caller's walk over S.sc[0 .. min(CR_T, len - c0)) follows, and behind it the
// tile's third barrier.
__device__ __forceinline__ void cr_tile(const CrShared &S, const CrTiles &T, const int c0, double *colscore)
{
    const DevProb &P = S.P;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int len = T.len, kind = T.kind, an = T.an, nm = T.nm;
    unsigned long long *mask = T.mask;
    int *last = T.last;
    DList zd; zd.p = S.zero_delta; zd.s = 1;
    const int c = c0 + tid;
    const bool live = c < len;
    const int cc = live ? c : len - 1;
    for (int j = 0; j < nm; ++j) {
        const bool ina = kind == 3 && j < an;
        const uint8_t r = ina ? res_at(P.a, cc)[j] : res_at(P.b, cc)[kind == 3 ? j - an : j];
        const unsigned long long m = __ballot(live && r > 1);
        if (lane == 0) mask[j * CR_W + wave] = m;
    }
    __syncthreads();
    if (live) {
        double s = sim2(P, c, c);
        if (kind == 3) {
            int *gl = S.gl;
            for (int j = 0; j < nm; ++j) gl[j * CR_T + tid] = cr_runlen(mask, last, j, c0, c, wave, lane);
            s = s + crg2(P, gl + tid, gl + an * CR_T + tid, CR_T, c, c, 0);
        } else if (kind == 1) {
            s = s + cr_newgap2(P, c, mask, last, c0, wave, lane);
        } else if (kind == 2) {
            s = s + newgap4(gfq_at(P.a, 0, c), zd, gfq_at(P.b, 1, c), zd) * P.basic_gop
                  + newgap4(gfq_at(P.b, 0, c), zd, gfq_at(P.a, 1, c), zd) * P.basic_gop;
        }
        S.sc[tid] = s;
        if (colscore) colscore[c] = s;
    }
    __syncthreads();
    for (int j = tid; j < nm; j += CR_T)
        for (int w = CR_W - 1; w >= 0; --w) {
            const unsigned long long m = mask[j * CR_W + w];
            if (m) { last[j] = c0 + w * 64 + (63 - __clzll((long long) m)) + 1; break; }
        }
}

extern "C" __global__ void __launch_bounds__(CR_T) g2g_consreg_kernel(const DevProb *probs, const ConsregArgs *args)
{
    extern __shared__ __align__(16) unsigned char cr_dyn[];
    __shared__ double sc[CR_T];
    __shared__ int gl[CR_NV_MEM * CR_T];
    __shared__ int2 zero_delta[2];
    __shared__ DevProb P;
    const CrShared S = {sc, gl, zero_delta, P};
    const ConsregArgs A = args[blockIdx.x];
    const CrTiles T = cr_begin(S, cr_dyn, &probs[blockIdx.x]);
    // the scan's scalars (consreg.cc:172-182; `sum` is only printed there)
    double scr = 0, mxv = 0;
    int rl = 0, rr = 0, nr = 0;
    __syncthreads();
    for (int c0 = 0; c0 < T.len; c0 += CR_T) {
        cr_tile(S, T, c0, A.colscore);
        if (threadIdx.x == 0) {
            const int n = T.len - c0 < CR_T ? T.len - c0 : CR_T;
            for (int k = 0; k < n; ++k) {
                const double s = S.sc[k];
                const int i = c0 + k;
                if (scr == 0 && s > 0) rl = i;
                scr += s;
                if (scr < 0) scr = 0;
                else if (scr >= A.vthr && scr > mxv) { mxv = scr; rr = i + 1; }
                if (mxv > 0 && (scr <= 0 || scr < mxv - A.vthr)) {
                    if (nr < A.cap) A.ranges[nr] = make_int2(rl, rr);
                    ++nr;
                    mxv = scr = 0;
                }
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (scr >= A.vthr) { if (nr < A.cap) A.ranges[nr] = make_int2(rl, rr); ++nr; }
        *A.nranges = nr;
    }
}

// ConservedT::mayfuse (consreg.cc:452-464): may_fuse_ng / _nv / _hf / _pf (:211-225, 276-298, 345-364, 408-424) walk the same column
// scores with another recurrence -- scr += s; a positive scr is set to 0; the walk breaks where scr < fthr -- and the pair fuses iff
// the walk reaches the last column.  One workgroup per test over the same tiles; when lane 0's walk breaks it leaves the column in
// LDS and the whole workgroup leaves behind the tile's barrier.
struct MayfuseArgs {
    double fthr;                      // Conserved2::fthr (consreg.cc:73), formed on the host
    int2 *out;                        // {fuse, stop_col}
};

extern "C" __global__ void __launch_bounds__(CR_T) g2g_mayfuse_kernel(const DevProb *probs, const MayfuseArgs *args)
{
    extern __shared__ __align__(16) unsigned char cr_dyn[];
    __shared__ double sc[CR_T];
    __shared__ int gl[CR_NV_MEM * CR_T];
    __shared__ int2 zero_delta[2];
    __shared__ DevProb P;
    const CrShared S = {sc, gl, zero_delta, P};
    __shared__ int stop_at;                                    // the column at which scr < fthr first held, -1 while the walk goes on
    const MayfuseArgs A = args[blockIdx.x];
    const CrTiles T = cr_begin(S, cr_dyn, &probs[blockIdx.x]);
    if (threadIdx.x == 0) stop_at = -1;
    double scr = 0;
    __syncthreads();
    for (int c0 = 0; c0 < T.len; c0 += CR_T) {
        cr_tile(S, T, c0, 0);
        if (threadIdx.x == 0) {
            const int n = T.len - c0 < CR_T ? T.len - c0 : CR_T;
            for (int k = 0; k < n; ++k) {
                scr += S.sc[k];
                if (scr > 0) scr = 0;
                if (scr < A.fthr) { stop_at = c0 + k; break; }
            }
        }
        __syncthreads();
        if (stop_at >= 0) break;                               // read by every lane behind the barrier: the exit is uniform
    }
    if (threadIdx.x == 0) *A.out = make_int2(stop_at < 0 ? 1 : 0, stop_at);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
namespace {
typedef std::vector<g2g_range> CrRanges;
// cmnrng(a, b, 0), src/css.cc:261-282: the intersection of two ascending lists of disjoint ranges, empty pieces dropped
CrRanges cr_cmnrng(const CrRanges &a, const CrRanges &b)
{
    CrRanges out;
    size_t i = 0, j = 0;
    while (i < a.size() && j < b.size()) {
        const bool a_low = a[i].right <= b[j].right;              // ll: the range that ends first
        const g2g_range &ll = a_low ? a[i] : b[j], &uu = a_low ? b[j] : a[i];
        if (ll.right >= uu.left) {
            g2g_range c;
            c.left = std::max(a[i].left, b[j].left);
            c.right = ll.right;
            if (c.right - c.left > 0) out.push_back(c);
        }
        if (a_low) ++i; else ++j;
    }
    return out;
}
// complerng(c, a), src/css.cc:313-336, with c the single range [left, right)
CrRanges cr_complerng(int left, int right, const CrRanges &r)
{
    CrRanges out;
    g2g_range b;
    b.left = left;
    for (const g2g_range &x : r) {
        b.right = x.left;
        if (b.left < b.right) out.push_back(b);
        b.left = x.right;
    }
    b.right = right;
    if (b.left < b.right) out.push_back(b);
    return out;
}
g2g_range *cr_hand_out(const CrRanges &r)
{
    g2g_range *p = (g2g_range *) malloc(sizeof(g2g_range) * (r.size() ? r.size() : 1));
    if (p && !r.empty()) memcpy(p, r.data(), sizeof(g2g_range) * r.size());
    return p;
}
double cr_now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// What g2g_constwo_batch and g2g_mayfuse_batch refuse in pair i, before the device is asked for anything; `what` is the reference's
// function, whose switch the message names.  nm: the members whose gap runs the kernel reads.
int cr_check_pair(const char *who, int i, const g2g_problem *p, const char *what, size_t *nm)
{
    int rc = G2G_OK;
    if (p->alnmode < G2G_NGP_ALB || p->alnmode > G2G_NTV_ALB) { rc = G2G_ERR_MODE; g2g_errorf(who, "pair %d: mode %d is not a banded mode (%s's switch reads the banded names only)", i, p->alnmode, what); }
    else if (p->a.npfq > 0 || p->b.npfq > 0) { rc = G2G_ERR_MODE; g2g_errorf(who, "pair %d: annotated (spliced) groups are not on this path", i); }
    else if (p->a.nils || p->b.nils) { rc = G2G_ERR_MODE; g2g_errorf(who, "pair %d: groups with discounted terminal gaps are not on this path", i); }
    else if (p->a.len != p->b.len || p->a.left != 0 || p->b.left != 0 || p->a.right != p->a.len || p->b.right != p->b.len) { rc = G2G_ERR_ARG; g2g_errorf(who, "pair %d: the two groups must have the same length and stand whole (%d and %d columns)", i, p->a.len, p->b.len); }
    else if (p->alnmode == G2G_NTV_ALB && p->a.many + p->b.many > CR_NV_MEM) { rc = G2G_ERR_MODE; g2g_errorf(who, "pair %d: a naive-record pair of %d members", i, p->a.many + p->b.many); }
    else if ((rc = check_problem(p)) != G2G_OK) g2g_errorf(who, "pair %d: not a problem of this library (status %d)", i, rc);
    if (rc != G2G_OK) return rc;
    const int kind = kind_of(p->alnmode);
    *nm = kind == 3 ? (size_t) p->a.many + p->b.many : kind == 1 ? (size_t) p->b.many : 0;
    return G2G_OK;
}
// the dynamic LDS of a launch whose largest pair reads nm_max members, [nm][CR_W] masks and [nm] last: refused beyond 48 KB
bool cr_lds_bytes(const char *who, size_t nm_max, size_t *lds)
{
    *lds = (nm_max * (8 * CR_W + 4) + 15) & ~(size_t) 15;
    if (*lds > 48 * 1024) { g2g_set_error("%s: a gap-free group of more than 1365 members on the _hf path", who); return false; }
    return true;
}

// n built pairs on the device, one workgroup each.  The inputs as g2g_batch_prepare packs them (arrays a device builder left in
// HBM are read where they lie) and nothing else: no DP state, no trace.  The block from the context's pool holds
// [DevProb n][args n][the problems' arrays] and, from out() on, out_bytes for the kernel to write.  The caller packs, fills its
// argument structs with addresses behind out(), uploads, launches on ctx->stream unless e is set, and fetches: `back` is then what
// lies behind out().  The block returns to the pool when the object goes.
struct CrPairs {
    g2g_ctx *ctx; const char *who; int n;
    Blob bl;                                                      // (the staging buffer goes back to the context with it)
    std::vector<DevProb> dp;
    std::vector<DevPatch> patches;
    size_t arg_size = 0, o_probs = 0, o_args = 0, in_bytes = 0, out_bytes = 0;
    char *dev = 0; size_t dev_cap = 0;
    bool timed = false;
    hipError_t e = hipSuccess;
    std::vector<char> back;
    CrPairs(g2g_ctx *c, const char *w, int n_) : ctx(c), who(w), n(n_), bl(c), dp((size_t) n_) {}
    ~CrPairs() { pool_give(ctx, dev, dev_cap); }
    char *out() const { return dev + in_bytes; }
    const DevProb *probs() const { return (const DevProb *) (dev + o_probs); }
    const void *args() const { return dev + o_args; }
    int pack(const g2g_problem *const *prob, size_t arg_size_, size_t out_bytes_)
    {
        arg_size = arg_size_;
        bl.grow(staging_estimate(ctx, n, prob) + arg_size * (size_t) n);
        o_probs = bl.put(0, 0);
        bl.extend(o_probs + sizeof(DevProb) * (size_t) n);
        o_args = bl.put(0, 0);
        bl.extend(o_args + arg_size * (size_t) n);
        for (int i = 0; i < n; ++i) pack_problem(bl, prob[i], dp[(size_t) i], patches);
        bl.flush();
        if (bl.oom) { g2g_set_error("%s: host staging buffer: out of (pinned) memory", who); return G2G_ERR_NOMEM; }
        in_bytes = (bl.size() + 255) & ~(size_t) 255;
        out_bytes = out_bytes_;
        dev = (char *) pool_take(ctx, in_bytes + out_bytes, &dev_cap);
        if (!dev) { g2g_set_error("%s: out of device memory", who); (void) hipGetLastError(); return G2G_ERR_NOMEM; }
        for (int i = 0; i < n; ++i) rebase_problem(dp[(size_t) i], dev);
        for (const DevPatch &pt : patches) *pt.field = pt.value;
        return G2G_OK;
    }
    // timing_switch: the diagnostic option that asks for device events around the kernel (tools/consreg_probe.py, tools/fuse_probe.py)
    void upload(const void *args, const char *timing_switch)
    {
        memcpy(bl.data() + o_probs, dp.data(), sizeof(DevProb) * (size_t) n);
        memcpy(bl.data() + o_args, args, arg_size * (size_t) n);
        e = hipMemcpyAsync(dev, bl.data(), bl.size(), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        timed = g2g_opt(ctx, timing_switch) != 0;
        if (e == hipSuccess && timed) e = hipEventRecord(ctx->ev[0], ctx->stream);
    }
    // everything behind the inputs comes back in one copy; ms_option: the kernel's time, summed over the calls since it was cleared
    int fetch(const char *ms_option)
    {
        if (e == hipSuccess && timed) e = hipEventRecord(ctx->ev[1], ctx->stream);
        back.resize(out_bytes);                                   // (here, not earlier: the kernel runs while the host clears these pages)
        if (e == hipSuccess) e = hipMemcpyAsync(back.data(), out(), out_bytes, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        else (void) hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess && timed) e = g2g_note_events(ctx, ms_option, ctx->ev[0], ctx->ev[1], true);
        if (e != hipSuccess) { g2g_errorf(who, "%s", hipGetErrorString(e)); (void) hipGetLastError(); return G2G_ERR_DEVICE; }
        return G2G_OK;
    }
};
}

// host only, no context: cmnrng (dissim = 0: the intersection of a and b) or complerng (dissim = 1: [0, len) without a; b is not
// read) on plain lists -- what g2g_consreg finishes with
extern "C" int g2g_ranges_combine(const g2g_range *a, int na, const g2g_range *b, int nb, int dissim, int len, g2g_range **out, int *nout)
{
    if (!out || !nout || na < 0 || nb < 0 || (na && !a) || (!dissim && nb && !b) || (dissim && len < 0)) return G2G_ERR_ARG;
    const CrRanges ra(a, a + na);
    CrRanges r;
    if (dissim) r = cr_complerng(0, len, ra);
    else r = cr_cmnrng(ra, CrRanges(b, b + nb));
    *out = cr_hand_out(r);
    *nout = (int) r.size();
    return *out ? G2G_OK : G2G_ERR_NOMEM;
}

extern "C" int g2g_constwo_batch(g2g_ctx *ctx, int n, g2g_pwdm *const *pw, double thr, g2g_range **ranges, int *nranges, double **colscore, int *status)
{
    const char *who = "g2g_constwo_batch";
    if (n < 0 || (n && (!pw || !ranges || !nranges))) { g2g_set_error("%s: bad argument", who); return G2G_ERR_ARG; }
    if (!(thr > 0)) { g2g_set_error("%s: thr must be positive", who); return G2G_ERR_ARG; }
    for (int i = 0; i < n; ++i) { ranges[i] = 0; nranges[i] = 0; if (colscore) colscore[i] = 0; if (status) status[i] = G2G_OK; }
    std::vector<const g2g_problem *> prob((size_t) n);
    std::vector<double> vthr((size_t) n);
    // behind the inputs: nranges[n], then every division's slot of ranges and, where asked for, its column scores
    std::vector<size_t> o_rng((size_t) n), o_col((size_t) n);
    size_t nm_max = 0, lds = 0, out_bytes = (4 * (size_t) n + 255) & ~(size_t) 255;
    for (int i = 0; i < n; ++i) {
        const g2g_problem *p = pw[i] ? g2g_pwdm_problem(pw[i]) : 0;
        g2g_spparams sp;
        if (!p || g2g_pwdm_spparams(pw[i], &sp) != G2G_OK) { g2g_set_error("%s: a NULL pair", who); return G2G_ERR_ARG; }
        size_t nm = 0;
        const int rc = cr_check_pair(who, i, p, "constwo", &nm);
        if (rc != G2G_OK) { if (status) status[i] = rc; return rc; }
        prob[(size_t) i] = p;
        vthr[(size_t) i] = sp.vab * thr;
        nm_max = std::max(nm_max, nm);
        const size_t len = (size_t) p->a.len, cap = len / 2 + 2;
        o_rng[(size_t) i] = out_bytes; out_bytes += (sizeof(int2) * cap + 15) & ~(size_t) 15;
        o_col[(size_t) i] = out_bytes; if (colscore) out_bytes += (8 * len + 15) & ~(size_t) 15;
    }
    if (!cr_lds_bytes(who, nm_max, &lds)) return G2G_ERR_MODE;
    if (!ctx) { g2g_set_error("%s: no context", who); return G2G_ERR_ARG; }
    if (!ctx->ok) return G2G_ERR_NODEVICE;
    HIPCHK(hipSetDevice(ctx->device));
    if (n == 0) return G2G_OK;
    CrPairs dv(ctx, who, n);
    int rc = dv.pack(prob.data(), sizeof(ConsregArgs), out_bytes);
    if (rc != G2G_OK) return rc;
    std::vector<ConsregArgs> ar((size_t) n);
    for (int i = 0; i < n; ++i) {
        ConsregArgs &a = ar[(size_t) i];
        a.vthr = vthr[(size_t) i];
        a.ranges = (int2 *) (dv.out() + o_rng[(size_t) i]); a.cap = prob[(size_t) i]->a.len / 2 + 2;
        a.nranges = (int *) dv.out() + i;
        a.colscore = colscore ? (double *) (dv.out() + o_col[(size_t) i]) : 0;
    }
    dv.upload(ar.data(), "CONSREG_TIMING");
    if (dv.e == hipSuccess) {
        hipLaunchKernelGGL(g2g_consreg_kernel, dim3((unsigned) n), dim3(CR_T), lds, ctx->stream, dv.probs(), (const ConsregArgs *) dv.args());
        dv.e = hipGetLastError();
    }
    rc = dv.fetch("CONSREG_KERNEL_MS");
    if (rc != G2G_OK) return rc;
    const char *back = dv.back.data();
    for (int i = 0; i < n && rc == G2G_OK; ++i) {
        const int len = prob[(size_t) i]->a.len, cap = len / 2 + 2;
        const int nr = ((const int *) back)[i];
        if (nr < 0 || nr > cap) { g2g_set_error("%s: a division produced more ranges than its slot holds", who); rc = G2G_ERR_DEVICE; break; }
        ranges[i] = (g2g_range *) malloc(sizeof(g2g_range) * (size_t) (nr ? nr : 1));
        if (!ranges[i]) { rc = G2G_ERR_NOMEM; break; }
        memcpy(ranges[i], back + o_rng[(size_t) i], sizeof(g2g_range) * (size_t) nr);
        nranges[i] = nr;
        if (colscore) {
            colscore[i] = (double *) malloc(8 * (size_t) len);
            if (!colscore[i]) { rc = G2G_ERR_NOMEM; break; }
            memcpy(colscore[i], back + o_col[(size_t) i], 8 * (size_t) len);
        }
    }
    if (rc != G2G_OK)
        for (int i = 0; i < n; ++i) { free(ranges[i]); ranges[i] = 0; nranges[i] = 0; if (colscore) { free(colscore[i]); colscore[i] = 0; } }
    return rc;
}

// ConservedT::mayfuse on n built pairs: the counterpart of g2g_constwo_batch (same packing, same refusals, all before the device is
// asked for).  fuse[i] 0 / 1, stop_col[i] the column at which scr < fthr first held or -1.
extern "C" int g2g_mayfuse_batch(g2g_ctx *ctx, int n, g2g_pwdm *const *pw, double u, double v, int *fuse, int *stop_col, int *status)
{
    const char *who = "g2g_mayfuse_batch";
    if (n < 0 || (n && (!pw || !fuse || !stop_col))) { g2g_set_error("%s: bad argument", who); return G2G_ERR_ARG; }
    if (!(u >= 0) || !(v >= 0)) { g2g_set_error("%s: u and v must not be negative", who); return G2G_ERR_ARG; }
    for (int i = 0; i < n; ++i) { fuse[i] = 0; stop_col[i] = -1; if (status) status[i] = G2G_OK; }
    std::vector<const g2g_problem *> prob((size_t) n);
    std::vector<double> fthr((size_t) n);
    size_t nm_max = 0, lds = 0;
    for (int i = 0; i < n; ++i) {
        const g2g_problem *p = pw[i] ? g2g_pwdm_problem(pw[i]) : 0;
        if (!p) { g2g_set_error("%s: a NULL pair", who); return G2G_ERR_ARG; }
        size_t nm = 0;
        const int rc = cr_check_pair(who, i, p, "mayfuse", &nm);
        if (rc != G2G_OK) { if (status) status[i] = rc; return rc; }
        prob[(size_t) i] = p;
        // fthr = (VTYPE) -((2 * localprm.u + localprm.v)) * a->sumwt * b->sumwt (consreg.cc:73): u and v are floats there, the cast
        // binds to the negated sum, the products run left to right in VTYPE = double
        const float uf = (float) u, vf = (float) v;
        fthr[(size_t) i] = (double) -((2 * uf + vf)) * p->a.sumwt * p->b.sumwt;
        nm_max = std::max(nm_max, nm);
    }
    if (!cr_lds_bytes(who, nm_max, &lds)) return G2G_ERR_MODE;
    if (!ctx) { g2g_set_error("%s: no context", who); return G2G_ERR_ARG; }
    if (!ctx->ok) return G2G_ERR_NODEVICE;
    HIPCHK(hipSetDevice(ctx->device));
    if (n == 0) return G2G_OK;
    CrPairs dv(ctx, who, n);
    int rc = dv.pack(prob.data(), sizeof(MayfuseArgs), (sizeof(int2) * (size_t) n + 255) & ~(size_t) 255);   // behind the inputs: {fuse, stop_col}[n]
    if (rc != G2G_OK) return rc;
    std::vector<MayfuseArgs> ar((size_t) n);
    for (int i = 0; i < n; ++i) { ar[(size_t) i].fthr = fthr[(size_t) i]; ar[(size_t) i].out = (int2 *) dv.out() + i; }
    dv.upload(ar.data(), "FUSE_TIMING");
    if (dv.e == hipSuccess) {
        hipLaunchKernelGGL(g2g_mayfuse_kernel, dim3((unsigned) n), dim3(CR_T), lds, ctx->stream, dv.probs(), (const MayfuseArgs *) dv.args());
        dv.e = hipGetLastError();
    }
    rc = dv.fetch("FUSE_KERNEL_MS");
    if (rc != G2G_OK) return rc;
    const int2 *back = (const int2 *) dv.back.data();
    for (int i = 0; i < n; ++i) {
        const int len = prob[(size_t) i]->a.len;
        if ((back[i].x != 0 && back[i].x != 1) || back[i].y < -1 || back[i].y >= len || (back[i].x == 1) != (back[i].y < 0)) {
            g2g_errorf(who, "pair %d came back as (%d, %d)", i, back[i].x, back[i].y);
            return G2G_ERR_DEVICE;
        }
        fuse[i] = back[i].x; stop_col[i] = back[i].y;
    }
    return G2G_OK;
}

namespace {
// a relation: groups of members and the tree over them (Ssrel: Subset + Ktree) as plain vectors
struct CrRel {
    std::vector<std::vector<int>> group;
    std::vector<int> left, right, parent, origin;
    std::vector<double> vol, cur;
    int fused = 0;
    int nn() const { return (int) left.size(); }
    int root() const { for (int k = 0; k < nn(); ++k) if (parent[(size_t) k] < 0) return k; return -1; }
};

// tree over nl leaves (leaves 0 .. nl - 1 without children, one root, every node reached once from it) and, when given, the subset:
// an error text or NULL.  post: the nodes in post-order, left before right
const char *cr_check_relation(const g2g_tree *tree, int nl, const g2g_subset *ss, int many, std::vector<int> *post)
{
    if (!tree || !tree->left || !tree->right || !tree->parent) return "bad argument";
    if (ss) {
        if (ss->num < 1 || ss->elms < ss->num || ss->elms > many || !ss->start || !ss->member) return "malformed subset";
        if (ss->start[0] != 0 || ss->start[ss->num] != ss->elms) return "malformed subset (start)";
        std::vector<char> seen((size_t) many, 0);
        for (int g = 0; g < ss->num; ++g) {
            if (ss->start[g + 1] <= ss->start[g] || ss->start[g + 1] > ss->elms) return "malformed subset (an empty group)";
            for (int k = ss->start[g]; k < ss->start[g + 1]; ++k) {
                const int m = ss->member[k];
                if (m < 0 || m >= many || seen[(size_t) m]) return "malformed subset (a member out of range or named twice)";
                seen[(size_t) m] = 1;
            }
        }
    }
    const int nn = tree->n_nodes;
    if (nn != 2 * nl - 1) return "the tree must have 2 * groups - 1 nodes";
    int root = -1;
    for (int k = 0; k < nn; ++k) {
        const int l = tree->left[k], r = tree->right[k], p = tree->parent[k];
        if (l < -1 || l >= nn || r < -1 || r >= nn || p < -1 || p >= nn || (k < nl ? (l != -1 || r != -1) : (l < 0 || r < 0 || l == r))) return "malformed tree";
        if (p < 0) { if (root >= 0) return "malformed tree (two roots)"; root = k; }
    }
    if (root < 0 || (nl > 1 && root < nl)) return "malformed tree (no root)";
    std::vector<char> seen((size_t) nn, 0);
    std::vector<std::pair<int, int>> st(1, std::make_pair(root, 0));
    int cnt = 0;
    while (!st.empty()) {
        const int k = st.back().first;
        if (st.back().second == 0) {
            if (seen[(size_t) k]) return "malformed tree (a node is reachable twice)";
            seen[(size_t) k] = 1; ++cnt;
            st.back().second = 1;
            if (tree->left[k] >= 0) {
                if (tree->parent[tree->left[k]] != k || tree->parent[tree->right[k]] != k) return "malformed tree (parent links)";
                st.push_back(std::make_pair(tree->right[k], 0)); st.push_back(std::make_pair(tree->left[k], 0));
            }
        } else {
            if (post) post->push_back(k);
            st.pop_back();
        }
    }
    if (cnt != nn) return "malformed tree (not every node hangs below the root)";
    return 0;
}

void cr_rel_from(CrRel &r, const g2g_tree *tree, int nl, const g2g_subset *ss)
{
    const size_t nn = (size_t) tree->n_nodes;
    r.left.assign(tree->left, tree->left + nn); r.right.assign(tree->right, tree->right + nn); r.parent.assign(tree->parent, tree->parent + nn);
    r.vol.assign(nn, 0.); r.cur.assign(nn, 0.);
    if (tree->vol) r.vol.assign(tree->vol, tree->vol + nn);
    if (tree->cur) r.cur.assign(tree->cur, tree->cur + nn);
    r.origin.resize(nn);
    for (size_t k = 0; k < nn; ++k) r.origin[k] = (int) k;
    r.group.assign((size_t) nl, std::vector<int>());
    for (int g = 0; g < nl; ++g) {
        if (ss) r.group[(size_t) g].assign(ss->member + ss->start[g], ss->member + ss->start[g + 1]);
        else r.group[(size_t) g].assign(1, g);
    }
    r.fused = 0;
}

// one fusing: a relation, a column range, and what the rounds found
struct CrFuseJob {
    const CrRel *rel = 0;
    int left = 0, right = 0;
    std::vector<int> state;                       // per node: -1 not tested (yet), 0 refused, 1 stands for one group (leaves from the start)
    std::vector<std::vector<int>> members;        // per node with state 1: its group, the leaves' members from left to right
};

struct CrBuildTimes { double build = 0, fuse = 0, host = 0; };

// sons of the member lists over the columns [left, right) of codes, built through the level-1 builders: Seq::extseq with every column
// kept, weights handed down / nfact = 1, a single member gets 1 (src/seq.cc:1096-1153)
struct CrSonSpec { const std::vector<int> *lst[2]; int left, right; };
int cr_build_pairs(g2g_ctx *ctx, const g2g_params *prm, int many, const uint8_t *codes, const double *weight, const std::vector<CrSonSpec> &spec, size_t b0, int nb,
                   std::vector<g2g_group *> &ga, std::vector<g2g_group *> &gb, std::vector<g2g_pwdm *> &pw, const char *who)
{
    ga.assign((size_t) nb, (g2g_group *) 0); gb.assign((size_t) nb, (g2g_group *) 0); pw.assign((size_t) nb, (g2g_pwdm *) 0);
    std::atomic<int> next(0), bad(0);
    auto work = [&]() {
        std::vector<uint8_t> c;
        std::vector<double> w;
        for (int k; (k = next.fetch_add(1)) < nb; ) {
            const CrSonSpec &sp = spec[b0 + (size_t) k];
            const int len = sp.right - sp.left;
            g2g_group *made[2] = {0, 0};
            for (int s = 0; s < 2; ++s) {
                const std::vector<int> &lst = *sp.lst[s];
                const int m = (int) lst.size();
                c.resize((size_t) len * m);
                for (int r = 0; r < len; ++r) for (int i = 0; i < m; ++i) c[(size_t) r * m + i] = codes[(size_t) (sp.left + r) * many + lst[(size_t) i]];
                w.clear();
                if (weight) for (int i = 0; i < m; ++i) w.push_back(m == 1 ? 1. : weight[lst[(size_t) i]]);
                made[s] = g2g_group_create(ctx, prm, m, len, c.data(), weight ? w.data() : 0);
            }
            ga[(size_t) k] = made[0]; gb[(size_t) k] = made[1];
            if (!made[0] || !made[1]) bad.store(1);
        }
    };
    unsigned nthr = std::thread::hardware_concurrency();
    if (nthr > 16) nthr = 16;
    if (nthr < 1) nthr = 1;
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nthr && (int) t < nb; ++t) { try { th.emplace_back(work); } catch (...) { break; } }
    work();
    for (auto &t : th) t.join();
    if (bad.load()) { g2g_set_error("%s: building a son failed", who); return G2G_ERR_ARG; }
    return g2g_pwdm_create_batch(ctx, prm, nb, ga.data(), gb.data(), 0, pw.data());
}
void cr_free_pairs(std::vector<g2g_group *> &ga, std::vector<g2g_group *> &gb, std::vector<g2g_pwdm *> &pw)
{
    for (size_t k = 0; k < pw.size(); ++k) { if (pw[k]) g2g_pwdm_free(pw[k]); if (ga[k]) g2g_group_free(ga[k]); if (gb[k]) g2g_group_free(gb[k]); }
    ga.clear(); gb.clear(); pw.clear();
}

// ConservedT::testssrel (consreg.cc:569-589) for several (relation, range) jobs at once, level by level: round r holds, of every job,
// the inner nodes whose two sons stand for one group each -- exactly the tests the post-order walk runs -- and is one
// g2g_mayfuse_batch (more where a round's residue codes exceed the chunk bound)
int cr_fuse_rounds(g2g_ctx *ctx, const g2g_params *prm, int many, const uint8_t *codes, const double *weight, std::vector<CrFuseJob> &jobs,
                   g2g_fuse_stats *stats, CrBuildTimes &tm, const char *who)
{
    for (CrFuseJob &j : jobs) {
        const CrRel &r = *j.rel;
        j.state.assign((size_t) r.nn(), -1);
        j.members.assign((size_t) r.nn(), std::vector<int>());
        for (size_t g = 0; g < r.group.size(); ++g) { j.state[g] = 1; j.members[g] = r.group[g]; }
    }
    size_t cap_codes = (size_t) 128 << 20, cap_n = 512;
    if (const char *o = g2g_opt(ctx, "FUSE_CHUNK")) { const int v = atoi(o); if (v >= 1) cap_n = (size_t) v; }
    for (;;) {
        const double t0 = cr_now();
        std::vector<std::pair<int, int>> cand;                       // (job, node)
        std::vector<CrSonSpec> spec;
        for (size_t ji = 0; ji < jobs.size(); ++ji) {
            CrFuseJob &j = jobs[ji];
            const CrRel &r = *j.rel;
            for (int k = (int) r.group.size(); k < r.nn(); ++k) {
                if (j.state[(size_t) k] != -1) continue;
                const int l = r.left[(size_t) k], rt = r.right[(size_t) k];
                if (j.state[(size_t) l] == 1 && j.state[(size_t) rt] == 1) {
                    cand.push_back(std::make_pair((int) ji, k));
                    CrSonSpec sp;
                    sp.lst[0] = &j.members[(size_t) l]; sp.lst[1] = &j.members[(size_t) rt]; sp.left = j.left; sp.right = j.right;
                    spec.push_back(sp);
                }
            }
        }
        tm.host += cr_now() - t0;
        if (cand.empty()) break;
        std::vector<int> fz(cand.size(), 0), sc(cand.size(), -1);
        for (size_t b0 = 0; b0 < cand.size(); ) {
            size_t nb = 0, load = 0;
            while (b0 + nb < cand.size() && nb < cap_n) {
                const CrSonSpec &sp = spec[b0 + nb];
                const size_t add = (sp.lst[0]->size() + sp.lst[1]->size()) * (size_t) (sp.right - sp.left);
                if (nb && load + add > cap_codes) break;
                load += add; ++nb;
            }
            std::vector<g2g_group *> ga, gb;
            std::vector<g2g_pwdm *> pw;
            const double t1 = cr_now();
            int rc = cr_build_pairs(ctx, prm, many, codes, weight, spec, b0, (int) nb, ga, gb, pw, who);
            const double t2 = cr_now();
            tm.build += t2 - t1;
            if (rc == G2G_OK) rc = g2g_mayfuse_batch(ctx, (int) nb, pw.data(), prm->u, prm->v, fz.data() + b0, sc.data() + b0, 0);
            tm.fuse += cr_now() - t2;
            cr_free_pairs(ga, gb, pw);
            if (rc != G2G_OK) return rc;
            if (stats) ++stats->launches;
            b0 += nb;
        }
        const double t3 = cr_now();
        for (size_t i = 0; i < cand.size(); ++i) {
            CrFuseJob &j = jobs[(size_t) cand[i].first];
            const CrRel &r = *j.rel;
            const int k = cand[i].second;
            if (stats) { ++stats->tests; stats->fused += fz[i]; }
            j.state[(size_t) k] = fz[i];
            if (fz[i]) {                                             // the right group's members are appended to the left group's
                std::vector<int> &m = j.members[(size_t) k];
                m = j.members[(size_t) r.left[(size_t) k]];
                const std::vector<int> &rm = j.members[(size_t) r.right[(size_t) k]];
                m.insert(m.end(), rm.begin(), rm.end());
            }
        }
        tm.host += cr_now() - t3;
    }
    return G2G_OK;
}

// what Ssrel::consregss hands back (consreg.cc:692-711) once the tests are known: the groups in leaf post-order and the tree
// ConservedT::rearrange makes (:667-689) -- a node that stands for a group becomes the leaf of that number, the other inner nodes get
// n, n + 1, ... in post-order, every other field is the old node's.  Nothing fused: the input relation again (the reference's NULL)
void cr_rearrange(const CrFuseJob &j, CrRel &out)
{
    const CrRel &r = *j.rel;
    const int k = (int) r.group.size();
    std::vector<int> tops;                                           // maximal nodes with state 1, in post-order
    std::vector<int> newid((size_t) r.nn(), -1);
    {   // pre-order with left first gives the groups from left to right
        std::vector<int> st(1, r.root());
        while (!st.empty()) {
            const int x = st.back(); st.pop_back();
            if (j.state[(size_t) x] == 1) { newid[(size_t) x] = (int) tops.size(); tops.push_back(x); continue; }
            st.push_back(r.right[(size_t) x]); st.push_back(r.left[(size_t) x]);
        }
    }
    const int n = (int) tops.size();
    if (n == k) { out = r; out.fused = 0; return; }
    out = CrRel();
    out.fused = 1;
    const size_t nn = (size_t) (2 * n - 1);
    out.left.assign(nn, -1); out.right.assign(nn, -1); out.parent.assign(nn, -1); out.origin.assign(nn, -1); out.vol.assign(nn, 0.); out.cur.assign(nn, 0.);
    for (int g = 0; g < n; ++g) out.group.push_back(j.members[(size_t) tops[(size_t) g]]);
    int ntid = n;
    // post-order over the nodes above the groups
    std::vector<std::pair<int, int>> st(1, std::make_pair(r.root(), 0));
    while (!st.empty()) {
        const int x = st.back().first;
        if (newid[(size_t) x] < 0 && st.back().second == 0) {
            st.back().second = 1;
            st.push_back(std::make_pair(r.right[(size_t) x], 0)); st.push_back(std::make_pair(r.left[(size_t) x], 0));
            continue;
        }
        if (newid[(size_t) x] < 0) newid[(size_t) x] = ntid++;
        const size_t t = (size_t) newid[(size_t) x];
        out.origin[t] = x;
        out.vol[t] = r.vol[(size_t) x]; out.cur[t] = r.cur[(size_t) x];
        if ((int) t >= n) {
            out.left[t] = newid[(size_t) r.left[(size_t) x]]; out.right[t] = newid[(size_t) r.right[(size_t) x]];
            out.parent[(size_t) out.left[t]] = out.parent[(size_t) out.right[t]] = (int) t;
        }
        st.pop_back();
    }
}

int cr_rel_hand_out(const CrRel &r, g2g_relation *o)
{
    memset(o, 0, sizeof *o);
    const size_t nn = (size_t) r.nn(), ng = r.group.size();
    size_t elms = 0;
    for (const auto &g : r.group) elms += g.size();
    o->fused = r.fused;
    o->ss.num = (int32_t) ng; o->ss.elms = (int32_t) elms;
    o->ss.start = (int32_t *) malloc(4 * (ng + 1)); o->ss.member = (int32_t *) malloc(4 * (elms ? elms : 1));
    o->n_nodes = (int32_t) nn;
    o->left = (int32_t *) malloc(4 * nn); o->right = (int32_t *) malloc(4 * nn); o->parent = (int32_t *) malloc(4 * nn); o->origin = (int32_t *) malloc(4 * nn);
    o->vol = (double *) malloc(8 * nn); o->cur = (double *) malloc(8 * nn);
    if (!o->ss.start || !o->ss.member || !o->left || !o->right || !o->parent || !o->origin || !o->vol || !o->cur) { g2g_relation_free(o); return G2G_ERR_NOMEM; }
    size_t at = 0;
    for (size_t g = 0; g < ng; ++g) { o->ss.start[g] = (int32_t) at; for (int m : r.group[g]) o->ss.member[at++] = m; }
    o->ss.start[ng] = (int32_t) at;
    for (size_t k = 0; k < nn; ++k) { o->left[k] = r.left[k]; o->right[k] = r.right[k]; o->parent[k] = r.parent[k]; o->origin[k] = r.origin[k]; o->vol[k] = r.vol[k]; o->cur[k] = r.cur[k]; }
    return G2G_OK;
}

int cr_mode_check(const g2g_params *prm, const char *who)
{
    if (prm->banded != 1) { g2g_set_error("%s: banded must be 1 (with algmode.bnd = 0 every mode falls into the switch's default branch)", who); return G2G_ERR_MODE; }
    if (prm->u0 > 0) { g2g_set_error("%s: ether scorers (u0 > 0) are not on this path", who); return G2G_ERR_MODE; }
    if ((float) prm->tgapf != 1.f) { g2g_set_error("%s: the terminal-gap discount is not on this path", who); return G2G_ERR_MODE; }
    return G2G_OK;
}
void cr_fuse_note(g2g_ctx *ctx, const CrBuildTimes &tm)
{
    g2g_note_ms(ctx, "FUSE_BUILD_MS", tm.build, false); g2g_note_ms(ctx, "FUSE_HOST_MS", tm.host, false);
}
int cr_consreg_run(g2g_ctx *ctx, const g2g_params *prm, double thr, int many, int len, const uint8_t *codes, const double *weight,
                   const g2g_tree *tree, const g2g_subset *groups, int dissim, g2g_range **out, int *nout, const char *who);
}

extern "C" void g2g_subset_free(g2g_subset *s)
{
    if (!s) return;
    free(s->start); free(s->member);
    memset(s, 0, sizeof *s);
}
extern "C" void g2g_relation_free(g2g_relation *r)
{
    if (!r) return;
    g2g_subset_free(&r->ss);
    free(r->left); free(r->right); free(r->parent); free(r->origin); free(r->vol); free(r->cur);
    memset(r, 0, sizeof *r);
}

// Ssrel::consregss (consreg.cc:692-711) on the columns [left, right)
extern "C" int g2g_consregss(g2g_ctx *ctx, const g2g_params *prm, int many, int len, const uint8_t *codes, const double *weight, const g2g_tree *tree,
                             const g2g_subset *groups, int left, int right, g2g_relation *out, g2g_fuse_stats *stats)
{
    const char *who = "g2g_consregss";
    if (stats) memset(stats, 0, sizeof *stats);
    if (!prm || !codes || !tree || !out || len < 1) { g2g_set_error("%s: bad argument", who); return G2G_ERR_ARG; }
    memset(out, 0, sizeof *out);
    if (many < 2) { g2g_set_error("%s: fewer than two members", who); return G2G_ERR_ARG; }
    if (left < 0 || right > len || left >= right) { g2g_errorf(who, "the range [%d, %d) is empty or leaves the %d columns", left, right, len); return G2G_ERR_ARG; }
    int rc = cr_mode_check(prm, who);
    if (rc != G2G_OK) return rc;
    const int nl = groups ? groups->num : many;
    if (const char *bad = cr_check_relation(tree, nl, groups, many, 0)) { g2g_errorf(who, "%s", bad); return G2G_ERR_ARG; }
    if (!ctx) { g2g_set_error("%s: no context", who); return G2G_ERR_ARG; }
    if (!ctx->ok) return G2G_ERR_NODEVICE;
    const bool timed = g2g_opt(ctx, "FUSE_TIMING") != 0;
    if (timed) ctx->opt.erase("FUSE_KERNEL_MS");
    CrRel rel;
    cr_rel_from(rel, tree, nl, groups);
    std::vector<CrFuseJob> jobs(1);
    jobs[0].rel = &rel; jobs[0].left = left; jobs[0].right = right;
    CrBuildTimes tm;
    rc = cr_fuse_rounds(ctx, prm, many, codes, weight, jobs, stats, tm, who);
    if (rc != G2G_OK) return rc;
    const double t0 = cr_now();
    CrRel res;
    cr_rearrange(jobs[0], res);
    rc = cr_rel_hand_out(res, out);
    tm.host += cr_now() - t0;
    if (timed) cr_fuse_note(ctx, tm);
    return rc;
}

// Ssrel::consreg over a relation with groups (consreg.cc:484-518): the leaves of `tree` are the groups
extern "C" int g2g_consreg_groups(g2g_ctx *ctx, const g2g_params *prm, double thr, int many, int len, const uint8_t *codes, const double *weight,
                                  const g2g_tree *tree, const g2g_subset *groups, int dissim, g2g_range **out, int *nout)
{
    const char *who = "g2g_consreg_groups";
    if (!prm || !codes || !tree || !out || !nout || len < 1) { g2g_set_error("%s: bad argument", who); return G2G_ERR_ARG; }
    const int nl = groups ? groups->num : many;
    if (many < 2 || nl < 2) { g2g_set_error("%s: fewer than two groups have no division into two sons", who); return G2G_ERR_ARG; }
    if (!(thr > 0)) { g2g_set_error("%s: thr must be positive", who); return G2G_ERR_ARG; }
    if (const char *bad = cr_check_relation(tree, nl, groups, many, 0)) { g2g_errorf(who, "%s", bad); return G2G_ERR_ARG; }
    return cr_consreg_run(ctx, prm, thr, many, len, codes, weight, tree, groups, dissim, out, nout, who);
}

extern "C" void g2g_refine_plan_free(g2g_refine_plan_t *p)
{
    if (!p) return;
    g2g_relation_free(&p->whole);
    for (int i = 0; i < p->nranges && p->range_rel; ++i) g2g_relation_free(&p->range_rel[i]);
    free(p->range_rel); free(p->ranges); free(p->at_left); free(p->at_right);
    memset(p, 0, sizeof *p);
}

// what IterMsa::preprrn decides before any Prrn is built (prrn5.cc:794-823)
// -- from singletons (groups NULL), or from a relation the caller brings: tree is then the tree over `groups`
static int cr_refine_plan(const char *who, g2g_ctx *ctx, const g2g_params *prm, double thr, int many, int len, const uint8_t *codes, const double *weight,
                          const g2g_tree *tree, const g2g_subset *groups, g2g_refine_plan_t *out)
{
    if (!prm || !codes || !tree || !out || len < 1) { g2g_set_error("%s: bad argument", who); return G2G_ERR_ARG; }
    memset(out, 0, sizeof *out);
    if (many < 2) { g2g_set_error("%s: fewer than two members", who); return G2G_ERR_ARG; }
    if (!(thr > 0)) { g2g_set_error("%s: thr must be positive", who); return G2G_ERR_ARG; }
    int rc = cr_mode_check(prm, who);
    if (rc != G2G_OK) return rc;
    const int nl = groups ? groups->num : many;
    if (const char *bad = cr_check_relation(tree, nl, groups, many, 0)) { g2g_errorf(who, "%s", bad); return G2G_ERR_ARG; }
    if (!ctx) { g2g_set_error("%s: no context", who); return G2G_ERR_ARG; }
    if (!ctx->ok) return G2G_ERR_NODEVICE;
    const bool timed = g2g_opt(ctx, "FUSE_TIMING") != 0;
    if (timed) ctx->opt.erase("FUSE_KERNEL_MS");
    CrBuildTimes tm;
    CrRel rel0, srl;
    cr_rel_from(rel0, tree, nl, groups);
    {   // rrl = consregss(infc); srl = rrl ? rrl : this
        std::vector<CrFuseJob> jobs(1);
        jobs[0].rel = &rel0; jobs[0].left = 0; jobs[0].right = len;
        rc = cr_fuse_rounds(ctx, prm, many, codes, weight, jobs, &out->stats, tm, who);
        if (rc != G2G_OK) return rc;
        cr_rearrange(jobs[0], srl);
    }
    rc = cr_rel_hand_out(srl, &out->whole);
    if (rc != G2G_OK) return rc;
    if ((int) srl.group.size() < 2) { out->status = G2G_PLAN_NOTHING_TO_REFINE; if (timed) cr_fuse_note(ctx, tm); return G2G_OK; }
    // atkrng = srl->consreg(msd, DISSIM)
    g2g_range *atk = 0;
    int natk = 0;
    {
        g2g_tree t;
        t.n_nodes = srl.nn(); t.left = srl.left.data(); t.right = srl.right.data(); t.parent = srl.parent.data(); t.vol = srl.vol.data(); t.cur = srl.cur.data();
        rc = cr_consreg_run(ctx, prm, thr, many, len, codes, weight, &t, &out->whole.ss, 1, &atk, &natk, who);
        if (rc != G2G_OK) { g2g_refine_plan_free(out); return rc; }
    }
    out->ranges = atk; out->nranges = natk;
    out->at_left = (int32_t *) calloc((size_t) (natk ? natk : 1), 4); out->at_right = (int32_t *) calloc((size_t) (natk ? natk : 1), 4);
    out->range_rel = (g2g_relation *) calloc((size_t) (natk ? natk : 1), sizeof(g2g_relation));
    if (!out->at_left || !out->at_right || !out->range_rel) { g2g_refine_plan_free(out); return G2G_ERR_NOMEM; }
    // per range: trl = srl->consregss(infc) inside the range -- the ranges' rounds run together
    std::vector<CrFuseJob> jobs((size_t) natk);
    for (int i = 0; i < natk; ++i) {
        jobs[(size_t) i].rel = &srl; jobs[(size_t) i].left = atk[i].left; jobs[(size_t) i].right = atk[i].right;
        out->at_left[i] = atk[i].left == 0; out->at_right[i] = atk[i].right == len;   // exgl / exgr are kept there (prrn5.cc:814-815)
    }
    if (natk) rc = cr_fuse_rounds(ctx, prm, many, codes, weight, jobs, &out->stats, tm, who);
    for (int i = 0; i < natk && rc == G2G_OK; ++i) {
        CrRel res;
        cr_rearrange(jobs[(size_t) i], res);
        if (!res.fused) for (size_t k = 0; k < res.origin.size(); ++k) res.origin[k] = (int) k;
        rc = cr_rel_hand_out(res, &out->range_rel[i]);
    }
    if (rc != G2G_OK) { g2g_refine_plan_free(out); return rc; }
    if (timed) cr_fuse_note(ctx, tm);
    return G2G_OK;
}

extern "C" int g2g_refine_plan(g2g_ctx *ctx, const g2g_params *prm, double thr, int many, int len, const uint8_t *codes, const double *weight,
                               const g2g_tree *tree, g2g_refine_plan_t *out)
{
    return cr_refine_plan("g2g_refine_plan", ctx, prm, thr, many, len, codes, weight, tree, NULL, out);
}

// include/g2g_groups.h: the plan started from the caller's relation instead of singletons
extern "C" int g2g_refine_plan_groups(g2g_ctx *ctx, const g2g_params *prm, double thr, int many, int len, const uint8_t *codes, const double *weight,
                                      const g2g_tree *tree, const g2g_subset *groups, g2g_refine_plan_t *out)
{
    if (!groups) { g2g_set_error("%s", "g2g_refine_plan_groups: bad argument"); return G2G_ERR_ARG; }
    return cr_refine_plan("g2g_refine_plan_groups", ctx, prm, thr, many, len, codes, weight, tree, groups, out);
}

extern "C" int g2g_consreg(g2g_ctx *ctx, const g2g_params *prm, double thr, int many, int len, const uint8_t *codes, const double *weight,
                           const g2g_tree *tree, int dissim, g2g_range **out, int *nout)
{
    const char *who = "g2g_consreg";
    if (!prm || !codes || !tree || !out || !nout || len < 1) { g2g_set_error("%s: bad argument", who); return G2G_ERR_ARG; }
    if (many < 3) { g2g_set_error("%s: fewer than three members have no division into two sons", who); return G2G_ERR_ARG; }
    if (!(thr > 0)) { g2g_set_error("%s: thr must be positive", who); return G2G_ERR_ARG; }
    if (tree->n_nodes != 2 * many - 1 || !tree->left || !tree->right || !tree->parent) { g2g_set_error("%s: the tree must have 2 * many - 1 nodes", who); return G2G_ERR_ARG; }
    return cr_consreg_run(ctx, prm, thr, many, len, codes, weight, tree, 0, dissim, out, nout, who);
}

namespace {
// the driver of g2g_consreg and g2g_consreg_groups: the leaves of the tree are the groups of `groups` (NULL: the members themselves)
int cr_consreg_run(g2g_ctx *ctx, const g2g_params *prm, double thr, int many, int len, const uint8_t *codes, const double *weight,
                   const g2g_tree *tree, const g2g_subset *groups, int dissim, g2g_range **out, int *nout, const char *who)
{
    const int nl = groups ? groups->num : many;
    if (prm->banded != 1) { g2g_set_error("%s: banded must be 1 (with algmode.bnd = 0 every mode falls into constwo's default branch)", who); return G2G_ERR_MODE; }
    if (prm->u0 > 0) { g2g_set_error("%s: ether scorers (u0 > 0) are not on this path", who); return G2G_ERR_MODE; }
    // (mkthick reads tgapf from the global alprm, src/mseq.cc:165-166: prm->tgapf stands for it here)
    if ((float) prm->tgapf != 1.f) { g2g_set_error("%s: the terminal-gap discount is not on this path", who); return G2G_ERR_MODE; }
    *out = 0; *nout = 0;
    // the branches: node r = 0 .. 2 many - 4 (Randiv::tree_tab, src/randiv.cc:120-156; the root's second child repeats its first);
    // bin2lst2g (:88-100) puts the members below the node into son 1 and the others into son 0, both ascending -- over a relation with
    // groups the leaves are groups: they are taken in ascending order and each hands over its members in its own order
    const int nn = tree->n_nodes, cycle = 2 * nl - 3;
    int root = -1;
    for (int k = 0; k < nn; ++k) {
        const int l = tree->left[k], r = tree->right[k], p = tree->parent[k];
        if (l < -1 || l >= nn || r < -1 || r >= nn || p < -1 || p >= nn || (k < nl ? (l != -1 || r != -1) : (l < 0 || r < 0 || l == r))) { g2g_set_error("%s: malformed tree", who); return G2G_ERR_ARG; }
        if (p < 0) { if (root >= 0) { g2g_set_error("%s: malformed tree (two roots)", who); return G2G_ERR_ARG; } root = k; }
    }
    if (root < nl) { g2g_set_error("%s: malformed tree (no root)", who); return G2G_ERR_ARG; }
    std::vector<std::vector<int>> inside((size_t) nn);
    {   // leaves below every node, children before parents (an explicit post-order walk; a node met twice is a malformed tree)
        std::vector<char> seen((size_t) nn, 0);
        std::vector<std::pair<int, int>> st(1, std::make_pair(root, 0));
        int cnt = 0;
        while (!st.empty()) {
            const int k = st.back().first;
            if (st.back().second == 0) {
                if (seen[(size_t) k]) { g2g_set_error("%s: malformed tree (a node is reachable twice)", who); return G2G_ERR_ARG; }
                seen[(size_t) k] = 1; ++cnt;
                st.back().second = 1;
                if (tree->left[k] >= 0) { st.push_back(std::make_pair(tree->right[k], 0)); st.push_back(std::make_pair(tree->left[k], 0)); }
                else inside[(size_t) k].push_back(k);
            } else {
                if (tree->left[k] >= 0) {
                    std::vector<int> &v = inside[(size_t) k];
                    v = inside[(size_t) tree->left[k]];
                    v.insert(v.end(), inside[(size_t) tree->right[k]].begin(), inside[(size_t) tree->right[k]].end());
                    std::sort(v.begin(), v.end());
                }
                st.pop_back();
            }
        }
        if (cnt != nn) { g2g_set_error("%s: malformed tree (not every node hangs below the root)", who); return G2G_ERR_ARG; }
    }
    std::vector<int> branches;
    for (int k = 0; k < nn; ++k) {
        if (k == root) continue;
        // the two children of the root cut the same branch: the later one is dropped (with the reference's numbering that is node 2 many - 3)
        if (tree->parent[k] == root && k == std::max(tree->left[root], tree->right[root])) continue;
        branches.push_back(k);
    }
    if ((int) branches.size() != cycle) { g2g_set_error("%s: malformed tree (parent links)", who); return G2G_ERR_ARG; }
    if (!ctx) { g2g_set_error("%s: no context", who); return G2G_ERR_ARG; }
    if (!ctx->ok) return G2G_ERR_NODEVICE;
    const bool timed = g2g_opt(ctx, "CONSREG_TIMING") != 0;
    if (timed) { ctx->opt.erase("CONSREG_KERNEL_MS"); }
    double t_build = 0, t_two = 0, t_host = 0;
    // chunks: the host arrays of a chunk's groups and their device twins stay within about 128 M residue codes
    size_t chunk = ((size_t) 128 << 20) / ((size_t) many * (size_t) len);
    chunk = std::max<size_t>(1, std::min<size_t>(chunk, 512));
    // the first chunk is small: where nothing is conserved across all branches the intersection is empty after a few divisions and
    // the reference stops there (consreg.cc:506) -- the result does not depend on where the loop stops
    size_t first = std::min<size_t>(chunk, 8);
    if (const char *o = g2g_opt(ctx, "CONSREG_CHUNK")) { const int v = atoi(o); if (v >= 1) first = chunk = (size_t) v; }
    const bool all_divisions = g2g_opt(ctx, "CONSREG_NO_EARLY_STOP") != 0;     // diagnostic switch (tools/consreg_probe.py): every division is scored
    if (all_divisions) first = chunk;
    CrRanges united(1);
    united[0].left = 0; united[0].right = len;
    int rc = G2G_OK;
    for (size_t b0 = 0, step = first; b0 < branches.size() && rc == G2G_OK; b0 += step, step = chunk) {
        const int nb = (int) std::min(step, branches.size() - b0);
        std::vector<g2g_group *> ga((size_t) nb, (g2g_group *) 0), gb((size_t) nb, (g2g_group *) 0);
        std::vector<g2g_pwdm *> pw((size_t) nb, (g2g_pwdm *) 0);
        const double t0 = cr_now();
        {   // Ssrel::dividseq: extseq(sons[s], lstbuf[s], CPY_SEQ + CPY_NBR) -- every column kept; weights handed down / nfact = 1, a
            // single member gets 1 (Seq::extseq, src/seq.cc:1096-1153)
            std::atomic<int> next(0);
            std::atomic<int> bad(0);
            auto work = [&]() {
                std::vector<uint8_t> c;
                std::vector<double> w;
                std::vector<char> in((size_t) nl);
                for (int k; (k = next.fetch_add(1)) < nb; ) {
                    const std::vector<int> &ins = inside[(size_t) branches[b0 + (size_t) k]];
                    std::fill(in.begin(), in.end(), 0);
                    for (int l : ins) in[(size_t) l] = 1;
                    std::vector<int> son[2];
                    for (int i = 0; i < nl; ++i) {
                        std::vector<int> &to = son[in[(size_t) i] ? 1 : 0];
                        if (groups) to.insert(to.end(), groups->member + groups->start[i], groups->member + groups->start[i + 1]);
                        else to.push_back(i);
                    }
                    const std::vector<int> *lst[2] = {&son[0], &son[1]};
                    g2g_group *made[2] = {0, 0};
                    for (int s = 0; s < 2; ++s) {
                        const int m = (int) lst[s]->size();
                        c.resize((size_t) len * m);
                        for (int r = 0; r < len; ++r) for (int i = 0; i < m; ++i) c[(size_t) r * m + i] = codes[(size_t) r * many + (*lst[s])[(size_t) i]];
                        w.clear();
                        if (weight) for (int i = 0; i < m; ++i) w.push_back(m == 1 ? 1. : weight[(*lst[s])[(size_t) i]]);
                        made[s] = g2g_group_create(ctx, prm, m, len, c.data(), weight ? w.data() : 0);
                    }
                    ga[(size_t) k] = made[0]; gb[(size_t) k] = made[1];
                    if (!made[0] || !made[1]) bad.store(1);
                }
            };
            unsigned nthr = std::thread::hardware_concurrency();
            if (nthr > 16) nthr = 16;
            if (nthr < 1) nthr = 1;
            std::vector<std::thread> th;
            for (unsigned t = 1; t < nthr && (int) t < nb; ++t) { try { th.emplace_back(work); } catch (...) { break; } }
            work();
            for (auto &t : th) t.join();
            if (bad.load()) { g2g_set_error("%s: building a son failed", who); rc = G2G_ERR_ARG; }
        }
        if (rc == G2G_OK) rc = g2g_pwdm_create_batch(ctx, prm, nb, ga.data(), gb.data(), 0, pw.data());
        const double t1 = cr_now();
        t_build += t1 - t0;
        std::vector<g2g_range *> rg((size_t) nb, (g2g_range *) 0);
        std::vector<int> nr((size_t) nb, 0);
        if (rc == G2G_OK) rc = g2g_constwo_batch(ctx, nb, pw.data(), thr, rg.data(), nr.data(), 0, 0);
        const double t2 = cr_now();
        t_two += t2 - t1;
        for (int k = 0; k < nb && rc == G2G_OK; ++k) {            // united = cmnrng(prv, rng, 0); the order does not matter
            united = cr_cmnrng(united, CrRanges(rg[(size_t) k], rg[(size_t) k] + nr[(size_t) k]));
        }
        t_host += cr_now() - t2;
        for (int k = 0; k < nb; ++k) { free(rg[(size_t) k]); if (pw[(size_t) k]) g2g_pwdm_free(pw[(size_t) k]); if (ga[(size_t) k]) g2g_group_free(ga[(size_t) k]); if (gb[(size_t) k]) g2g_group_free(gb[(size_t) k]); }
        if (united.empty() && !all_divisions) break;                // (consreg.cc:506)
    }
    if (rc != G2G_OK) return rc;
    const double t3 = cr_now();
    if (dissim) united = cr_complerng(0, len, united);
    *out = cr_hand_out(united);
    *nout = (int) united.size();
    t_host += cr_now() - t3;
    if (timed) { g2g_note_ms(ctx, "CONSREG_BUILD_MS", t_build, false); g2g_note_ms(ctx, "CONSREG_CONSTWO_MS", t_two, false); g2g_note_ms(ctx, "CONSREG_HOST_MS", t_host, false); }
    return *out ? G2G_OK : G2G_ERR_NOMEM;
}
}
