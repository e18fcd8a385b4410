// g2g_kmer.hip -- k-mer composition distances between unaligned single sequences: what the reference's DistMat(Seq**, nn) gets
// from calcdist_kmer (src/phyl.cc:515-528, src/qdiv.cc:245-282) when algmode.any == Composition (src/prrn5.cc:976-979), and what
// AdjacentMat::dist_kmer computes per candidate pair (src/adjmat.cc:90-97).
//
//   words    Kcomp::makeHash (qdiv.cc:61-80) with the continuous seed bitmask(k) (Bitpat_wq::word / flaw, bitpat.cc:168-185): the
//            scan reads the residues left .. right - k - 1 (its end pointer is at(right - width)), and counts a word wherever the
//            last k residues read were all elementary (the 20 amino acids, or A C G T) -- an ungapped sequence of elementary
//            residues has max(0, (right - left) - 2 k + 1) words.  A word is the base-Nalpha number of its residues' classes
//            (Nalpha 20 / 4); which class gets which digit changes no result, here digit = code - ALA, and A C G T = 0 1 2 3.
//            Any other residue (X, B, Z, Sec, N and the other ambiguity codes, gap, nil) breaks the word: the reference reads
//            table entries it never wrote for them (bitpat.cc:76-86), here no word containing one is counted.
//   profile  the sorted (word, count) list of a sequence (Kcomp::Kcomp: Dhash::press + qsort, qdiv.cc:82-90), Unq entries, T words
//   pair     qdiv (qdiv.cc:179-232, many == 1): s = sum over shared words of min(count_a, count_b), f = s / min(Ta, Tb), then the
//            closed form of the DistMes (src/aln.h:54); the stored distance is 100 * qdiv (kcmp_main, qdiv.cc:239)
//
// The device computes integers only -- three per pair: s, Ta, Tb -- so any correct schedule gives the same bits; the doubles are
// formed on the host (g2g_kmer_dist_from_counts) in the reference's operation order.
//
// Kernel mapping.
//   g2g_kmer_profile_kernel    ONE WORKGROUP PER SEQUENCE.  The window's residues become digits in LDS (0xFF: not elementary);
//       every word position reads its k digits from there (k <= 15 LDS bytes: the validity of a position needs no scan over the
//       sequence); invalid positions and the padding get 0xFFFFFFFF, which no word can be while Nalpha^k < 2^32.  A bitonic
//       network sorts the power-of-two array in LDS; a run head finds its count by an upper-bound search in the sorted array and
//       its place in the list by a workgroup prefix sum.  Lists lie in HBM at a fixed stride per sequence (its number of word
//       positions, known to the host), keys and counts in two arrays.
//   g2g_kmer_profile_spec_kernel   the same for g2g_kmer_dist_batch_spec: a caller's class table (staged in LDS) instead of the full
//       alphabet, base nalpha, and a seed -- a word position reads its digits at the offsets of the seed's '1's (one 32-bit mask,
//       a kernel argument; the continuous seed of k is the k low bits).  Sort, compaction and lists are the same.
//   g2g_kmer_allpairs_kernel   a workgroup keeps the list of member j in LDS and takes up to KM_CHUNK partners i < j, one partner
//       per wave at a time: each lane loads consecutive entries of the partner's list (coalesced), binary-searches its key in
//       LDS and adds the smaller count; the wave reduces with shuffles and lane 0 stores.  Results of a workgroup are consecutive
//       in the reference's elem() order, j (j - 1) / 2 + i.
//   g2g_kmer_pairlist_kernel   an index-pair list: one wave per pair, the shorter list streamed, the longer searched in HBM / L2.
// Plain launches on the context's stream: no atomics, nothing waits on another workgroup.
#include <hip/hip_runtime.h>
#include <math.h>

#define G2G_KMER_MAX_WINDOW 16384       // the most word positions, (right - left) - 2 k + 1, a sequence may have: 64 KB of keys in LDS
#define G2G_KMER_MAX_SEQS 4096          // all-pairs form (g2g_ktree_from_dist takes as many)
#define KM_THREADS 1024
#define KM_PAIR_THREADS 256
#define KM_CHUNK 64                     // partners per workgroup of the all-pairs kernel
#define KM_NOWORD 0xFFFFFFFFu

struct KmSeq { long long res; long long list; int words; int pad; };   // first residue of the window in the pool, first list entry, word positions

__device__ __forceinline__ unsigned km_digit(const unsigned c, const int molc)
{
    if (molc == 1) return c - 3u < 20u ? c - 3u : 0xFFu;              // ALA 3 .. VAL 22 (src/cmn.h:111-114)
    return c == 2u ? 0u : c == 3u ? 1u : c == 5u ? 2u : c == 9u ? 3u : 0xFFu;   // A C G T: the IUPAC bit codes + 1
}

extern "C" __global__ void __launch_bounds__(KM_THREADS) g2g_kmer_profile_kernel(const uint8_t *pool, const KmSeq *seqs, const int molc, const int k,
                                                                                 unsigned *keys, int *cnts, int2 *meta)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char km_lds[];
    const int tid = threadIdx.x;
    const KmSeq sq = seqs[blockIdx.x];
    const int W = sq.words;
    if (W <= 0) {                                                     // (the whole workgroup: no barrier is skipped by a part of it)
        if (tid == 0) meta[blockIdx.x] = make_int2(0, 0);
        return;
    }
    int N = 2;
    while (N < W) N <<= 1;
    unsigned *key = (unsigned *) km_lds;                              // N keys | 32 wave sums | W + k - 1 digits
    int *wsum = (int *) (key + N);
    unsigned char *dig = (unsigned char *) (wsum + 32);
    const unsigned nalpha = molc == 1 ? 20u : 4u;
    const int nres = W + k - 1;
    for (int i = tid; i < nres; i += KM_THREADS) dig[i] = (unsigned char) km_digit(pool[sq.res + i], molc);
    __syncthreads();
    for (int p = tid; p < N; p += KM_THREADS) {
        unsigned w = 0, bad = p < W ? 0u : 1u;
        if (!bad)
            for (int q = 0; q < k; ++q) {
                const unsigned d = dig[p + q];
                bad |= d >> 7;
                w = w * nalpha + d;
            }
        key[p] = bad ? KM_NOWORD : w;
    }
    __syncthreads();
    for (int size = 2; size <= N; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (N >> 1); t += KM_THREADS) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const unsigned a = key[i], b = key[j];
                if ((a > b) == ((i & size) == 0)) { key[i] = b; key[j] = a; }
            }
            __syncthreads();
        }
    // run heads: thread t looks at the E consecutive entries from t * E
    const int E = N > KM_THREADS ? N / KM_THREADS : 1, base = tid * E;
    int c = 0;
    if (base < N)
        for (int e = 0; e < E; ++e) {
            const int i = base + e;
            const unsigned v = key[i];
            c += v != KM_NOWORD && (i == 0 || key[i - 1] != v);
        }
    const int lane = tid & 63, wave = tid >> 6;
    int inc = c;
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(inc, d, 64);
        if (lane >= d) inc += y;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int o = inc - c;
    for (int w = 0; w < wave; ++w) o += wsum[w];
    if (base < N)
        for (int e = 0; e < E; ++e) {
            const int i = base + e;
            const unsigned v = key[i];
            if (v != KM_NOWORD && (i == 0 || key[i - 1] != v)) {
                int lo = i + 1, n = N - lo;                           // the first entry above v
                while (n > 0) {
                    const int half = n >> 1;
                    if (key[lo + half] <= v) { lo += half + 1; n -= half + 1; } else n = half;
                }
                keys[sq.list + o] = v;                                // o < Unq <= W: inside this sequence's stride
                cnts[sq.list + o] = lo - i;
                ++o;
            }
        }
    if (tid == 0) {
        int unq = 0;
        for (int w = 0; w < KM_THREADS / 64; ++w) unq += wsum[w];
        int lo = 0, n = N;                                            // T: the first KM_NOWORD
        while (n > 0) {
            const int half = n >> 1;
            if (key[lo + half] != KM_NOWORD) { lo += half + 1; n -= half + 1; } else n = half;
        }
        meta[blockIdx.x] = make_int2(unq, lo);
    }
}

// The second half of g2g_kmer_profile_kernel, word for word, for the kernel below: the N keys in LDS (a power of two; KM_NOWORD
// behind the words) are sorted, the run heads become this sequence's (word, count) list, meta = (Unq, T).  The whole workgroup
// calls it, after the barrier behind the last key written.  (g2g_kmer_profile_kernel keeps its own copy: routed through this
// function its code object came out a few instructions different, and g2g_kmer_dist_batch is to stay as measured.)
__device__ __forceinline__ void km_sort_emit(unsigned *key, int *wsum, const int N, const KmSeq sq, unsigned *keys, int *cnts, int2 *meta)
{
    const int tid = threadIdx.x;
    for (int size = 2; size <= N; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (N >> 1); t += KM_THREADS) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const unsigned a = key[i], b = key[j];
                if ((a > b) == ((i & size) == 0)) { key[i] = b; key[j] = a; }
            }
            __syncthreads();
        }
    // run heads: thread t looks at the E consecutive entries from t * E
    const int E = N > KM_THREADS ? N / KM_THREADS : 1, base = tid * E;
    int c = 0;
    if (base < N)
        for (int e = 0; e < E; ++e) {
            const int i = base + e;
            const unsigned v = key[i];
            c += v != KM_NOWORD && (i == 0 || key[i - 1] != v);
        }
    const int lane = tid & 63, wave = tid >> 6;
    int inc = c;
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(inc, d, 64);
        if (lane >= d) inc += y;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int o = inc - c;
    for (int w = 0; w < wave; ++w) o += wsum[w];
    if (base < N)
        for (int e = 0; e < E; ++e) {
            const int i = base + e;
            const unsigned v = key[i];
            if (v != KM_NOWORD && (i == 0 || key[i - 1] != v)) {
                int lo = i + 1, n = N - lo;                           // the first entry above v
                while (n > 0) {
                    const int half = n >> 1;
                    if (key[lo + half] <= v) { lo += half + 1; n -= half + 1; } else n = half;
                }
                keys[sq.list + o] = v;                                // o < Unq <= W: inside this sequence's stride
                cnts[sq.list + o] = lo - i;
                ++o;
            }
        }
    if (tid == 0) {
        int unq = 0;
        for (int w = 0; w < KM_THREADS / 64; ++w) unq += wsum[w];
        int lo = 0, n = N;                                            // T: the first KM_NOWORD
        while (n > 0) {
            const int half = n >> 1;
            if (key[lo + half] != KM_NOWORD) { lo += half + 1; n -= half + 1; } else n = half;
        }
        meta[blockIdx.x] = make_int2(unq, lo);
    }
}

// The general case (g2g_kmer_dist_batch_spec): a caller's class table and a seed.  seed: bit o is set where the seed string has a
// '1' at offset o (width <= 32; the continuous seed of k is the k low bits), so the offsets are wave-uniform and need no table.
// sq.words counts with the width: (right - left) - 2 width + 1, and the word at position p examines the digits p + o.
extern "C" __global__ void __launch_bounds__(KM_THREADS) g2g_kmer_profile_spec_kernel(const uint8_t *pool, const KmSeq *seqs, const uint8_t *classes,
                                                                                      const unsigned nalpha, const int width, const unsigned seed,
                                                                                      unsigned *keys, int *cnts, int2 *meta)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char km_lds[];
    const int tid = threadIdx.x;
    const KmSeq sq = seqs[blockIdx.x];
    const int W = sq.words;
    if (W <= 0) {                                                     // (the whole workgroup: no barrier is skipped by a part of it)
        if (tid == 0) meta[blockIdx.x] = make_int2(0, 0);
        return;
    }
    int N = 2;
    while (N < W) N <<= 1;
    unsigned *key = (unsigned *) km_lds;                              // N keys | 32 wave sums | 256 B class table | W + width - 1 digits
    int *wsum = (int *) (key + N);
    unsigned char *tab = (unsigned char *) (wsum + 32);
    unsigned char *dig = tab + 256;
    if (tid < 256) tab[tid] = classes[tid];
    __syncthreads();
    const int nres = W + width - 1;
    for (int i = tid; i < nres; i += KM_THREADS) {
        const unsigned c = tab[pool[sq.res + i]];
        dig[i] = (unsigned char) (c < nalpha ? c : 0xFFu);             // a class >= nalpha breaks the word where the seed examines it
    }
    __syncthreads();
    for (int p = tid; p < N; p += KM_THREADS) {
        unsigned w = 0, bad = p < W ? 0u : 1u;
        if (!bad)
            for (unsigned m = seed; m; m &= m - 1) {                  // the '1's left to right
                const unsigned d = dig[p + __ffs(m) - 1];
                bad |= d >> 7;
                w = w * nalpha + d;
            }
        key[p] = bad ? KM_NOWORD : w;
    }
    __syncthreads();
    km_sort_emit(key, wsum, N, sq, keys, cnts, meta);
}

// sum over the words of B that A holds of min(count_A, count_B), by one wave; the same value in every lane
__device__ __forceinline__ int km_wave_shared(const unsigned *ak, const int *ac, const int na, const unsigned *bk, const int *bc, const int nb, const int lane)
{
    int s = 0;
    for (int t = lane; t < nb; t += 64) {
        const unsigned kb = bk[t];
        const int cb = bc[t];
        int lo = 0, n = na;
        while (n > 0) {
            const int half = n >> 1;
            if (ak[lo + half] < kb) { lo += half + 1; n -= half + 1; } else n = half;
        }
        if (lo < na && ak[lo] == kb) s += min(ac[lo], cb);
    }
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
    return s;
}

extern "C" __global__ void __launch_bounds__(KM_PAIR_THREADS) g2g_kmer_allpairs_kernel(const unsigned *keys, const int *cnts, const KmSeq *seqs, const int2 *meta,
                                                                                       int *out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char km_lds[];
    const int j = blockIdx.y, i0 = blockIdx.x * KM_CHUNK;
    if (i0 >= j) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int2 mj = meta[j];
    unsigned *kj = (unsigned *) km_lds;                               // Unq_j keys | Unq_j counts (the launch gives 8 bytes per word position)
    int *cj = (int *) (kj + mj.x);
    const long long lj = seqs[j].list;
    for (int t = tid; t < mj.x; t += KM_PAIR_THREADS) { kj[t] = keys[lj + t]; cj[t] = cnts[lj + t]; }
    __syncthreads();
    const int i1 = min(j, i0 + KM_CHUNK);
    for (int i = i0 + wave; i < i1; i += KM_PAIR_THREADS / 64) {
        const int2 mi = meta[i];
        const long long li = seqs[i].list;
        const int s = km_wave_shared(kj, cj, mj.x, keys + li, cnts + li, mi.x, lane);
        if (lane == 0) {
            int *o = out + 3 * ((size_t) j * (j - 1) / 2 + i);       // elem(i, j), cmn.h:115-117
            o[0] = s; o[1] = mi.y; o[2] = mj.y;
        }
    }
}

extern "C" __global__ void __launch_bounds__(KM_PAIR_THREADS) g2g_kmer_pairlist_kernel(const unsigned *keys, const int *cnts, const KmSeq *seqs, const int2 *meta,
                                                                                       const int npairs, const int *ia, const int *ib, int *out)
{
    const int lane = threadIdx.x & 63;
    const long long p = (long long) blockIdx.x * (KM_PAIR_THREADS / 64) + (threadIdx.x >> 6);
    if (p >= npairs) return;                                          // (a whole wave; the kernel has no barrier)
    const int a = ia[p], b = ib[p];
    const int2 ma = meta[a], mb = meta[b];
    const long long la = seqs[a].list, lb = seqs[b].list;
    const int s = ma.x >= mb.x ? km_wave_shared(keys + la, cnts + la, ma.x, keys + lb, cnts + lb, mb.x, lane)
                               : km_wave_shared(keys + lb, cnts + lb, mb.x, keys + la, cnts + la, ma.x, lane);
    if (lane == 0) { int *o = out + 3 * p; o[0] = s; o[1] = ma.y; o[2] = mb.y; }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
namespace {
enum { KM_QFdiv, KM_QFidn, KM_QCdiv, KM_QCidn, KM_QJuCa, KM_Qpamd, KM_NJuCa };   // DistMes, src/aln.h:54
const double km_outofrange = 1024;                                    // OUTOFRANGE
double km_jukcan(double nid)                                          // divseq.cc:107-113
{
    if (nid <= 0.) return (0.);
    nid = 1. - 4./3. * nid;
    if (nid <= 0.) return (km_outofrange);
    return (-3./4. * log(nid));
}
double km_jukcanpro(double nid)                                       // divseq.cc:115-121
{
    if (nid <= 0.) return (0.);
    nid = 1. - 20./19. * nid;
    if (nid <= 0.) return (km_outofrange);
    return (-19./20. * log(nid));
}
double km_pamcorrect(double x)                                        // divseq.cc:123-126 with corr_mhits == 0
{
    if (x <= 0) return (0);
    return (100. * x);
}
// what both entries come down to.  width / seed: the seed (bit o: a '1' at offset o; the continuous seed of k is its k low bits);
// p0, p1: the row of qdiv's param; classes: only where spec (the spec entry's profile kernel)
struct KmPlan { int molc, k, measure, width; unsigned nalpha, seed; double p0, p1; bool spec; uint8_t classes[256]; };
// the row of param (qdiv.cc:181-186, 214-222): by Nalpha as given and by Ktuple, whatever the seed
void km_row(KmPlan &pl)
{
    static const double param[4][2] = {{0.92042, 0.18677}, {0.34576, 0.07108}, {0.22333, 0.03164}, {0.18704, 0.00501}};   // d314 d414 d514 d420
    const int r = pl.nalpha == 14 && pl.k >= 3 && pl.k <= 5 ? pl.k - 3 : 3;
    pl.p0 = param[r][0]; pl.p1 = param[r][1];
}
// qdiv, qdiv.cc:202-231, with many == 1 on both sides
double km_qdiv(const int s, const int ta, const int tb, const int measure, const double p0, const double p1)
{
    double f = (double) ta;                                           // TtlKmers / many, exact
    const double e = (double) tb;
    f = f < e ? f : e;                                                // min(f, e) * a->many * b->many
    f = (double) s / f;                                               // 0 / 0 for a member without a word: NaN, as in the reference
    double d = 1. - f;
    switch (measure) {
        case KM_QFdiv: return (d);
        case KM_QFidn: return (f);
        case KM_NJuCa: return km_jukcan(d);
        default: break;
    }
    f = p0 * log((p1 + f) / (p1 + 1.)) + 1.;
    d = 1. - f;
    switch (measure) {
        case KM_QCidn: return (f);
        case KM_QJuCa: return km_jukcanpro(d);
        case KM_Qpamd: return km_pamcorrect(d) / 100.;
        default: break;
    }
    return (d);
}
// the parameters taken literally (resetqdiv's swapping of one molecule's defaults for the other's, qdiv.cc:45-57, is not reproduced).
// k: the reference forms (queue * nalpha + c) % TabSize in 32-bit unsigned arithmetic (bitpat.cc:183), so its words are the true
// words only while Nalpha^(k + 1) <= 2^32: protein k <= 6, DNA k <= 15 (MaxBitPat = 16 bounds k as well)
bool km_params(const char *who, const g2g_kmer_params *kp, KmPlan &pl)
{
    if (!kp) { g2g_set_error("%s: no parameters", who); return false; }
    if (kp->molc != 1 && kp->molc != 2) { g2g_set_error("%s: molc is 1 (protein) or 2 (DNA)", who); return false; }
    const int k = kp->k ? kp->k : kp->molc == 1 ? 5 : 10;             // def_wcp_aa / def_wcp_nc, qdiv.cc:32-33
    const int measure = kp->measure != -1 ? kp->measure : kp->molc == 1 ? KM_Qpamd : KM_QJuCa;
    if (k < 1 || k > (kp->molc == 1 ? 6 : 15)) { g2g_set_error("%s: k outside 1 .. 6 (protein) / 1 .. 15 (DNA)", who); return false; }
    if (measure < 0 || measure > 6) { g2g_set_error("%s: measure outside -1 .. 6", who); return false; }
    if (kp->reserved) { g2g_set_error("%s: reserved is not 0 (reduced alphabets and spaced seeds are not on this path)", who); return false; }
    pl.molc = kp->molc; pl.k = pl.width = k; pl.measure = measure;
    pl.nalpha = kp->molc == 1 ? 20u : 4u; pl.seed = (1u << k) - 1u; pl.spec = false;
    km_row(pl);
    return true;
}
// g2g_kmer_spec.  The words must be the true ones: the reference's continuous queue is (queue * nalpha + c) % nalpha^k in 32 bits
// (bitpat.cc:183), its spaced word a plain 32-bit sum (bitpat.cc:191-199), and KM_NOWORD must stay no word.  The batch entry wants
// the classes too; the closed form does not look at them.
bool km_spec(const char *who, const g2g_kmer_spec *sp, const bool batch, KmPlan &pl)
{
    if (!sp) { g2g_set_error("%s: no parameters", who); return false; }
    if (sp->molc != 1 && sp->molc != 2) { g2g_set_error("%s: molc is 1 (protein) or 2 (DNA)", who); return false; }
    const int full = sp->molc == 1 ? 20 : 4;
    const int k = sp->k ? sp->k : sp->molc == 1 ? 5 : 10;
    const int measure = sp->measure != -1 ? sp->measure : sp->molc == 1 ? KM_Qpamd : KM_QJuCa;
    const int nalpha = sp->nalpha ? sp->nalpha : full;
    if (nalpha < 2 || nalpha > full) { g2g_set_error("%s: nalpha is 0 or 2 .. 20 (protein) / 2 .. 4 (DNA)", who); return false; }
    if (k < 1 || k > 15) { g2g_set_error("%s: k outside 1 .. 15", who); return false; }
    if (measure < 0 || measure > 6) { g2g_set_error("%s: measure outside -1 .. 6", who); return false; }
    if (sp->reserved) { g2g_set_error("%s: reserved is not 0", who); return false; }
    int width = k, weight = k;
    unsigned seed = (1u << k) - 1u;
    if (sp->seed) {
        const size_t n = strlen(sp->seed);
        if (n < 1 || n > 32) { g2g_set_error("%s: seed: a string of 1 .. 32 characters '0' / '1'", who); return false; }
        width = (int) n; weight = 0; seed = 0;
        for (int o = 0; o < width; ++o) {
            if (sp->seed[o] != '0' && sp->seed[o] != '1') { g2g_set_error("%s: seed: only '0' and '1'", who); return false; }
            if (sp->seed[o] == '1') { seed |= 1u << o; ++weight; }
        }
        if (sp->seed[0] != '1' || sp->seed[width - 1] != '1') { g2g_set_error("%s: seed: the first and the last character are '1'", who); return false; }
        if (weight > 15) { g2g_set_error("%s: seed: weight above 15", who); return false; }
    }
    unsigned long long tab = 1;                                       // continuous: nalpha^(k + 1) <= 2^32; seed string: nalpha^weight < 2^32
    for (int q = 0; q < (sp->seed ? weight : k + 1) && tab <= (1ULL << 32); ++q) tab *= (unsigned) nalpha;
    if (sp->seed ? tab >= (1ULL << 32) : tab > (1ULL << 32)) {
        if (sp->seed) g2g_set_error("%s: seed: nalpha^weight is not below 2^32", who);
        else g2g_set_error("%s: k: nalpha^(k + 1) is above 2^32", who);
        return false;
    }
    pl.molc = sp->molc; pl.k = k; pl.measure = measure; pl.width = width; pl.nalpha = (unsigned) nalpha; pl.seed = seed; pl.spec = true;
    km_row(pl);
    if (!batch) return true;
    if (!sp->classes) {
        if (nalpha != full) { g2g_set_error("%s: an nalpha below the full alphabet needs classes", who); return false; }
        for (unsigned c = 0; c < 256; ++c)                              // the full alphabet: ALA 3 .. VAL 22 (src/cmn.h:111-114); A C G T
            pl.classes[c] = sp->molc == 1 ? (c - 3u < 20u ? c - 3u : 0xFFu) : c == 2u ? 0u : c == 3u ? 1u : c == 5u ? 2u : c == 9u ? 3u : 0xFFu;
        return true;
    }
    if (sp->nclasses < 1 || sp->nclasses > 256) { g2g_set_error("%s: nclasses outside 1 .. 256", who); return false; }
    memset(pl.classes, 0xFF, sizeof pl.classes);                      // codes >= nclasses break the word
    memcpy(pl.classes, sp->classes, (size_t) sp->nclasses);
    return true;
}
int km_from_counts(const char *who, const KmPlan &pl, int npairs, const int32_t *counts, double *dist)
{
    if (npairs < 0 || (npairs && (!counts || !dist))) { g2g_set_error("%s: bad argument", who); return G2G_ERR_ARG; }
    for (int p = 0; p < npairs; ++p) {
        const int32_t *c = counts + 3 * (size_t) p;
        if (c[0] < 0 || c[1] < 0 || c[2] < 0 || c[0] > (c[1] < c[2] ? c[1] : c[2])) {
            g2g_errorf(who, "pair %d: counts %d %d %d are no s <= min(Ta, Tb)", p, c[0], c[1], c[2]);
            return G2G_ERR_ARG;
        }
        dist[p] = 100. * km_qdiv(c[0], c[1], c[2], pl.measure, pl.p0, pl.p1);   // kcmp_main, qdiv.cc:239
    }
    return G2G_OK;
}
int km_batch(const char *who, g2g_ctx *ctx, const KmPlan &pl, int nseq, const g2g_dseq *seqs, int npairs, const int32_t *ia, const int32_t *ib,
             double *dist, int32_t *counts);
}

extern "C" int g2g_kmer_dist_from_counts(const g2g_kmer_params *kp, int npairs, const int32_t *counts, double *dist)
{
    KmPlan pl;
    if (!km_params("g2g_kmer_dist_from_counts", kp, pl)) return G2G_ERR_ARG;
    return km_from_counts("g2g_kmer_dist_from_counts", pl, npairs, counts, dist);
}

extern "C" int g2g_kmer_dist_from_counts_spec(const g2g_kmer_spec *sp, int npairs, const int32_t *counts, double *dist)
{
    KmPlan pl;
    if (!km_spec("g2g_kmer_dist_from_counts_spec", sp, false, pl)) return G2G_ERR_ARG;
    return km_from_counts("g2g_kmer_dist_from_counts_spec", pl, npairs, counts, dist);
}

extern "C" int g2g_kmer_dist_batch(g2g_ctx *ctx, const g2g_kmer_params *kp, int nseq, const g2g_dseq *seqs, int npairs,
                                   const int32_t *ia, const int32_t *ib, double *dist, int32_t *counts)
{
    KmPlan pl;
    if (!km_params("g2g_kmer_dist_batch", kp, pl)) return G2G_ERR_ARG;
    return km_batch("g2g_kmer_dist_batch", ctx, pl, nseq, seqs, npairs, ia, ib, dist, counts);
}

extern "C" int g2g_kmer_dist_batch_spec(g2g_ctx *ctx, const g2g_kmer_spec *sp, int nseq, const g2g_dseq *seqs, int npairs,
                                        const int32_t *ia, const int32_t *ib, double *dist, int32_t *counts)
{
    KmPlan pl;
    if (!km_spec("g2g_kmer_dist_batch_spec", sp, true, pl)) return G2G_ERR_ARG;
    return km_batch("g2g_kmer_dist_batch_spec", ctx, pl, nseq, seqs, npairs, ia, ib, dist, counts);
}

namespace {
int km_batch(const char *who, g2g_ctx *ctx, const KmPlan &pl, int nseq, const g2g_dseq *seqs, int npairs, const int32_t *ia, const int32_t *ib,
             double *dist, int32_t *counts)
{
    if (!seqs || !dist || (!ia) != (!ib)) { g2g_set_error("%s: null argument", who); return G2G_ERR_ARG; }
    const bool all = !ia;
    if (nseq < 2 || npairs < 0) { g2g_set_error("%s: nseq >= 2 and npairs >= 0", who); return G2G_ERR_ARG; }
    if (all && (nseq > G2G_KMER_MAX_SEQS || (long long) npairs != (long long) nseq * (nseq - 1) / 2)) {
        g2g_set_error("%s: all pairs: nseq <= 4096 and npairs = nseq (nseq - 1) / 2", who);
        return G2G_ERR_ARG;
    }
    if (!all)
        for (int p = 0; p < npairs; ++p)
            if (ia[p] < 0 || ia[p] >= nseq || ib[p] < 0 || ib[p] >= nseq) {
                g2g_errorf(who, "pair %d: index %d or %d outside 0 .. %d", p, ia[p], ib[p], nseq - 1);
                return G2G_ERR_ARG;
            }
    // the pool holds each sequence's window, left .. right - 1; the word positions give the list strides
    std::vector<KmSeq> hs((size_t) nseq);
    size_t pool = 0, lists = 0;
    int wmax = 0;
    for (int i = 0; i < nseq; ++i) {
        const g2g_dseq &s = seqs[i];
        if ((!s.res && s.right > s.left) || s.left < 0 || s.right < s.left || s.right > s.len) {
            g2g_errorf(who, "sequence %d: no residues, or not 0 <= left <= right <= len", i);
            return G2G_ERR_ARG;
        }
        const long long w = std::max(0LL, (long long) (s.right - s.left) - 2 * pl.width + 1);
        if (w > G2G_KMER_MAX_WINDOW) {
            g2g_errorf(who, "sequence %d has %lld word positions, more than %d", i, w, G2G_KMER_MAX_WINDOW);
            return G2G_ERR_ARG;
        }
        hs[i].res = (long long) pool; hs[i].list = (long long) lists; hs[i].words = (int) w; hs[i].pad = 0;
        pool += ((size_t) (s.right - s.left) + 15) & ~(size_t) 15;
        lists += (size_t) w;
        wmax = std::max(wmax, (int) w);
    }
    if (!ctx) { g2g_set_error("%s: no context", who); return G2G_ERR_ARG; }
    if (!ctx->ok) return G2G_ERR_NODEVICE;
    HIPCHK(hipSetDevice(ctx->device));
    if (npairs == 0) return G2G_OK;
    auto al = [](size_t v) { return (v + 255) & ~(size_t) 255; };
    // device image: pool | seqs | ia | ib | class table (uploaded) | keys | cnts | meta | out
    const size_t o_seq = al(pool), o_ia = al(o_seq + sizeof(KmSeq) * nseq), o_ib = al(o_ia + (all ? 0 : 4 * (size_t) npairs)),
                 o_tab = al(o_ib + (all ? 0 : 4 * (size_t) npairs)), o_key = al(o_tab + (pl.spec ? sizeof pl.classes : 0)), o_cnt = al(o_key + 4 * lists), o_meta = al(o_cnt + 4 * lists),
                 o_out = al(o_meta + 8 * (size_t) nseq), total = o_out + 12 * (size_t) npairs;
    std::vector<char> img(o_key, 0);
    for (int i = 0; i < nseq; ++i)
        if (seqs[i].right > seqs[i].left) memcpy(img.data() + hs[i].res, seqs[i].res + seqs[i].left, (size_t) (seqs[i].right - seqs[i].left));
    memcpy(img.data() + o_seq, hs.data(), sizeof(KmSeq) * nseq);
    if (!all) { memcpy(img.data() + o_ia, ia, 4 * (size_t) npairs); memcpy(img.data() + o_ib, ib, 4 * (size_t) npairs); }
    if (pl.spec) memcpy(img.data() + o_tab, pl.classes, sizeof pl.classes);
    std::vector<int32_t> own;
    if (!counts) { own.resize(3 * (size_t) npairs); counts = own.data(); }
    char *dev = 0;
    HIPCHK(hipMalloc((void **) &dev, total));
    hipError_t e = hipMemcpyAsync(dev, img.data(), o_key, hipMemcpyHostToDevice, ctx->stream);
    const bool timed = g2g_opt(ctx, "KMER_TIMING") != 0;              // diagnostic switch: device events around each kernel (tools/kmer_probe.py)
    const KmSeq *dseq = (const KmSeq *) (dev + o_seq);
    unsigned *dkey = (unsigned *) (dev + o_key);
    int *dcnt = (int *) (dev + o_cnt);
    int2 *dmeta = (int2 *) (dev + o_meta);
    if (e == hipSuccess && timed) e = hipEventRecord(ctx->ev[0], ctx->stream);
    if (e == hipSuccess) {
        int n2 = 2;
        while (n2 < wmax) n2 <<= 1;
        const size_t lds = 4 * (size_t) n2 + 128 + (pl.spec ? sizeof pl.classes : 0) + (((size_t) wmax + pl.width + 15) & ~(size_t) 15);
        const void *fn = pl.spec ? (const void *) g2g_kmer_profile_spec_kernel : (const void *) g2g_kmer_profile_kernel;
        if (lds > 64 * 1024) e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
        if (e == hipSuccess) {
            if (pl.spec)
                hipLaunchKernelGGL(g2g_kmer_profile_spec_kernel, dim3(nseq), dim3(KM_THREADS), lds, ctx->stream, (const uint8_t *) dev, dseq,
                                   (const uint8_t *) (dev + o_tab), pl.nalpha, pl.width, pl.seed, dkey, dcnt, dmeta);
            else
                hipLaunchKernelGGL(g2g_kmer_profile_kernel, dim3(nseq), dim3(KM_THREADS), lds, ctx->stream, (const uint8_t *) dev, dseq, pl.molc, pl.k,
                                   dkey, dcnt, dmeta);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess && timed) e = hipEventRecord(ctx->ev[1], ctx->stream);
    if (e == hipSuccess && timed) e = hipEventRecord(ctx->ev[2], ctx->stream);
    if (e == hipSuccess && all) {
        const size_t lds = 8 * (size_t) std::max(wmax, 1);
        if (lds > 64 * 1024) e = hipFuncSetAttribute((const void *) g2g_kmer_allpairs_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(g2g_kmer_allpairs_kernel, dim3((nseq - 1 + KM_CHUNK - 1) / KM_CHUNK, nseq), dim3(KM_PAIR_THREADS), lds, ctx->stream,
                               (const unsigned *) dkey, (const int *) dcnt, dseq, (const int2 *) dmeta, (int *) (dev + o_out));
            e = hipGetLastError();
        }
    } else if (e == hipSuccess) {
        const int wpb = KM_PAIR_THREADS / 64;
        hipLaunchKernelGGL(g2g_kmer_pairlist_kernel, dim3((npairs + wpb - 1) / wpb), dim3(KM_PAIR_THREADS), 0, ctx->stream, (const unsigned *) dkey,
                           (const int *) dcnt, dseq, (const int2 *) dmeta, npairs, (const int *) (dev + o_ia), (const int *) (dev + o_ib), (int *) (dev + o_out));
        e = hipGetLastError();
    }
    if (e == hipSuccess && timed) e = hipEventRecord(ctx->ev[3], ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(counts, dev + o_out, 12 * (size_t) npairs, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess && timed) {                                   // read back as options KMER_PROFILE_MS / KMER_PAIRS_MS (g2g_get_option)
        const char *name[2] = {"KMER_PROFILE_MS", "KMER_PAIRS_MS"};
        for (int h = 0; h < 2 && e == hipSuccess; ++h) e = g2g_note_events(ctx, name[h], ctx->ev[2 * h], ctx->ev[2 * h + 1], false);
    }
    (void) hipFree(dev);
    if (e != hipSuccess) { g2g_errorf(who, "%s", hipGetErrorString(e)); (void) hipGetLastError(); return G2G_ERR_DEVICE; }
    return km_from_counts(who, pl, npairs, counts, dist);
}
}
