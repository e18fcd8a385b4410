// g2g_ktree_groups.hip -- the weighting tree over groups the caller brings: IterMsa::phyl_pwt with ss->num < ss->elms (reference
// src/prrn5.cc:333-391).  include/g2g_groups.h states the entry points; this file is included by g2g_engine.hip behind
// g2g_ktree.hip, whose pair kernel, kt_dist and tree builder it uses.
//
// The group form of pairdvn (src/divseq.cc:65-105) walks, per column, every i of A (outer) against every j of B (inner) with
// counters gsi[i] shared by all j and gsj[j] shared by all i.  mch, mmc and unp are the sums of the pairwise counts; gap is not.
// Entering a column let  g[i] = nj x (i's gap run ending just before the column),  h[j] = the sum over j's current gap run of the
// residues A had in those columns,  a[i] / b[j] = "is a gap here",  ra = residues of A here,  R(i) = residues of A among the
// members before i.  Inside the column gsi[i] is g[i] + j while a[i] holds (it grows by one per inner step) and g[i] at j = 0,
// 0 behind it, otherwise; gsj[j] is h[j] + R(i) while b[j] holds and h[j] at i = 0, 0 behind it, otherwise.  Hence
//   gap += [a[0]]   #{j residue : g[0] + j <= h[j]}          (T1)   + [!b[0]]  #{i >= 1 : a[i] and g[i] == 0}        (T2)
//        + [b[0]]   #{i residue : g[i] >= h[0] + R(i)}       (T3)   + [ra > 0] #{j >= 1 : b[j] and h[j] == 0}        (T4)
// and then g[i] = a[i] ? g[i] + nj : 0,  h[j] = b[j] ? h[j] + ra : 0.  T1 and T4 are sums over the members of B of terms that
// read, of A, only ra, a[0] and g[0]; T2 and T3 are sums over the members of A of terms that read, of B, only b[0] and h[0].
//
// Mapping.  The members are laid out in the order of the groups' lists (slot p; group g owns the slots gstart[g] .. gstart[g+1]),
// so a group is a run of slots and a pair of slots p < p' of one group is that group's pair in list order.
//   1. g2g_msa_div_kernel (unchanged) on the slots: the counts of every pair of members.
//   2. g2g_grp_cols_kernel: one lane per (column, group): res[column][group] = the group's residues in the column and
//      R[column][slot] = those before the slot -- a walk over the group's bytes of one row.
//   3. g2g_grp_gap_kernel: ONE LANE PER (slot, other group q), 256 slots of one q to a workgroup.  The lane walks the columns
//      serially with two counters in registers: as a member of B (q < its group) h[j] and the gap run of A's first member, as a
//      member of A (q > its group) its own gap run and h[0] of B's first member -- and counts T1 + T4, or T2 + T3.  Per column it
//      reads its own code and R (consecutive bytes / shorts over the lanes) and, the same for the whole workgroup, q's first
//      member's code and res; KG_CHUNK columns are fetched before they are walked.  No LDS, no atomics, no waiting on other
//      workgroups.  The work is len x many x (num - 1) steps -- not len x sum ni nj.
//   4. g2g_grp_reduce_kernel: one wave per group pair sums the ni x nj member-pair counts of step 1 and the ni + nj partial gap
//      counts of step 3 (lanes strided over them, shuffles down the wave) and forms dist with kt_dist.
// All integers: the sums are exact whatever their order.
#include "../../include/g2g_groups.h"

#define KG_CHUNK 8
#define KG_THREADS 256

extern "C" __global__ void __launch_bounds__(KG_THREADS) g2g_grp_cols_kernel(const uint8_t *codes, const int many, const int len, const int num,
                                                                             const int *gstart, unsigned short *res, unsigned short *R)
{
    const size_t idx = (size_t) blockIdx.x * KG_THREADS + threadIdx.x;
    if (idx >= (size_t) len * num) return;
    const int c = (int) (idx / num), g = (int) (idx % num);
    const size_t row = (size_t) c * many;
    int cnt = 0;
    for (int p = gstart[g], e = gstart[g + 1]; p < e; ++p) {
        R[row + p] = (unsigned short) cnt;
        cnt += codes[row + p] > 1;
    }
    res[idx] = (unsigned short) cnt;
}

// One column of a lane's walk.  isB: the lane's member belongs to B (A = q); s1: the h counter (h[j], or h[0] of B's first member),
// s2: the run counter (A's first member's, or the lane's own).  x / f: the lane's member / q's first member is a gap here.
__device__ __forceinline__ void kg_column(int &gap, int &s1, int &s2, const bool isB, const int pos, const int mul,
                                          const bool x, const bool f, const int rq, const int rown, const int R)
{
    const int lhs = mul * s2 + (isB ? pos : 0), rhs = s1 + (isB ? 0 : R);
    const bool c1 = f && !x && (isB ? lhs <= rhs : lhs >= rhs);                                   // T1 | T3
    const bool c2 = x && pos >= 1 && (isB ? (rq > 0 && s1 == 0) : (!f && s2 == 0));               // T4 | T2
    gap += (int) c1 + (int) c2;
    const bool u = isB ? x : f, w = isB ? f : x;
    s1 = u ? s1 + (isB ? rq : rown) : 0;
    s2 = w ? s2 + 1 : 0;
}

extern "C" __global__ void __launch_bounds__(KG_THREADS) g2g_grp_gap_kernel(const uint8_t *codes, const int many, const int len, const int num,
                                                                            const int *gstart, const int *grp_of, const unsigned short *res,
                                                                            const unsigned short *R, int *part)
{
    const int p = blockIdx.x * KG_THREADS + threadIdx.x, q = blockIdx.y;
    if (p >= many) return;
    const int G = grp_of[p];
    int gap = 0;
    if (G != q) {
        const bool isB = q < G;
        const int pos = p - gstart[G], first = gstart[q];
        const int mul = isB ? gstart[G + 1] - gstart[G] : gstart[q + 1] - first;                  // nj: the size of B
        int s1 = 0, s2 = 0, c0 = 0;
        for (; c0 + KG_CHUNK <= len; c0 += KG_CHUNK) {
            int xv[KG_CHUNK], fv[KG_CHUNK], rqv[KG_CHUNK], rov[KG_CHUNK], Rv[KG_CHUNK];
#pragma unroll
            for (int k = 0; k < KG_CHUNK; ++k) {
                const size_t row = (size_t) (c0 + k) * many, rrow = (size_t) (c0 + k) * num;
                xv[k] = codes[row + p]; fv[k] = codes[row + first];
                rqv[k] = res[rrow + q]; rov[k] = res[rrow + G]; Rv[k] = R[row + p];
            }
#pragma unroll
            for (int k = 0; k < KG_CHUNK; ++k) kg_column(gap, s1, s2, isB, pos, mul, xv[k] <= 1, fv[k] <= 1, rqv[k], rov[k], Rv[k]);
        }
        for (; c0 < len; ++c0) {
            const size_t row = (size_t) c0 * many, rrow = (size_t) c0 * num;
            kg_column(gap, s1, s2, isB, pos, mul, codes[row + p] <= 1, codes[row + first] <= 1, res[rrow + q], res[rrow + G], R[row + p]);
        }
    }
    part[(size_t) q * many + p] = gap;
}

extern "C" __global__ void __launch_bounds__(64) g2g_grp_reduce_kernel(const int *pcounts, const int *part, const int *gstart, const int many,
                                                                       double *dist, int *counts)
{
    const int k = blockIdx.x, l = blockIdx.y;
    if (k >= l) return;
    const int sa = gstart[k], ni = gstart[k + 1] - sa, sb = gstart[l], nj = gstart[l + 1] - sb, t0 = threadIdx.x;
    int mch = 0, mmc = 0, unp = 0, gap = 0;
    for (int t = t0; t < ni * nj; t += 64) {
        const int i = sa + t / nj, j = sb + t % nj;                  // i < j: k < l and the groups' slots ascend
        const int4 v = *(const int4 *) (pcounts + 4 * ((size_t) j * (j - 1) / 2 + i));
        mch += v.x; mmc += v.y; unp += v.z;
    }
    for (int t = t0; t < ni; t += 64) gap += part[(size_t) l * many + sa + t];
    for (int t = t0; t < nj; t += 64) gap += part[(size_t) k * many + sb + t];
    for (int d = 32; d > 0; d >>= 1) {
        mch += __shfl_down(mch, d, 64); mmc += __shfl_down(mmc, d, 64);
        unp += __shfl_down(unp, d, 64); gap += __shfl_down(gap, d, 64);
    }
    if (t0 == 0) {
        const size_t e = (size_t) l * (l - 1) / 2 + k;
        const KtCount c = {mch, mmc, unp, gap, 0, 0};
        dist[e] = kt_dist(c);
        int4 o; o.x = mch; o.y = mmc; o.z = unp; o.w = gap;
        *(int4 *) (counts + 4 * e) = o;
    }
}

// groups partition 0 .. many - 1, every group has a member, and no pair's counters can pass INT_MAX
static int kg_check_groups(const char *who, int many, int len, const g2g_subset *ss)
{
    if (!ss || !ss->start || !ss->member || ss->num < 2 || ss->num > many || ss->elms != many || ss->start[0] != 0 || ss->start[ss->num] != many) {
        g2g_errorf(who, "the groups must be at least two and partition the %d members", many);
        return G2G_ERR_ARG;
    }
    std::vector<char> seen((size_t) many, 0);
    int big[2] = {-1, -1};                                            // the two largest groups: the pair whose counters go highest
    for (int g = 0; g < ss->num; ++g) {
        const int s = ss->start[g], e = ss->start[g + 1];
        if (s >= e || e > many) { g2g_errorf(who, "group %d is empty or its bounds do not ascend", g); return G2G_ERR_ARG; }
        for (int k = s; k < e; ++k) {
            const int m = ss->member[k];
            if (m < 0 || m >= many || seen[m]) { g2g_errorf(who, "group %d: member %d is out of range or listed twice", g, m); return G2G_ERR_ARG; }
            seen[m] = 1;
        }
        auto size = [&](int h) { return h < 0 ? 0 : ss->start[h + 1] - ss->start[h]; };
        if (size(g) > size(big[0])) { big[1] = big[0]; big[0] = g; }
        else if (size(g) > size(big[1])) big[1] = g;
    }
    const long long top = (long long) len * (ss->start[big[0] + 1] - ss->start[big[0]]) * (ss->start[big[1] + 1] - ss->start[big[1]]);
    if (top >= (1LL << 31)) {
        g2g_errorf(who, "groups %d and %d: len x ni x nj = %lld does not fit the reference's int counters", std::min(big[0], big[1]), std::max(big[0], big[1]), top);
        return G2G_ERR_ARG;
    }
    return G2G_OK;
}

// The device part: group distances / counts and, where slot_dist is given, the divergences of all pairs of slots (members in the
// order of the groups' lists; (p < p') at p' (p' - 1) / 2 + p).
static int kg_divergence(const char *who, g2g_ctx *ctx, int many, int len, const uint8_t *codes, const g2g_subset *ss,
                         double *dist, int32_t *counts, double *slot_dist)
{
    HIPCHK(hipSetDevice(ctx->device));
    const int num = ss->num;
    const size_t nb = (size_t) many * len, npm = (size_t) many * (many - 1) / 2, npg = (size_t) num * (num - 1) / 2;
    std::vector<uint8_t> slots(nb);                                   // the MSA with its members in list order
    for (int c = 0; c < len; ++c) {
        const uint8_t *src = codes + (size_t) c * many;
        uint8_t *dst = slots.data() + (size_t) c * many;
        for (int p = 0; p < many; ++p) dst[p] = src[ss->member[p]];
    }
    std::vector<int> tab((size_t) num + 1 + many);                    // gstart, then the group of every slot
    for (int g = 0; g <= num; ++g) tab[g] = ss->start[g];
    for (int g = 0; g < num; ++g) for (int p = ss->start[g]; p < ss->start[g + 1]; ++p) tab[(size_t) num + 1 + p] = g;
    auto al = [](size_t v) { return (v + 255) & ~(size_t) 255; };
    const size_t o_tab = al(nb), o_res = al(o_tab + 4 * tab.size()), o_R = al(o_res + 2 * (size_t) len * num), o_part = al(o_R + 2 * nb),
                 o_pdist = al(o_part + 4 * (size_t) num * many), o_pcnt = al(o_pdist + 8 * npm), o_dist = al(o_pcnt + 16 * npm),
                 o_cnt = al(o_dist + 8 * npg), total = o_cnt + 16 * npg;
    char *dev = 0;
    HIPCHK(hipMalloc((void **) &dev, total));
    hipError_t e = hipMemcpyAsync(dev, slots.data(), nb, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dev + o_tab, tab.data(), 4 * tab.size(), hipMemcpyHostToDevice, ctx->stream);
    const bool timed = g2g_opt(ctx, "KTREE_TIMING") != 0;            // diagnostic switch: device events around the kernels (tools/ktree_groups_probe.py)
    if (e == hipSuccess && timed) e = hipEventRecord(ctx->ev[0], ctx->stream);
    const uint8_t *d_codes = (const uint8_t *) dev;
    const int *d_gstart = (const int *) (dev + o_tab), *d_grp = d_gstart + num + 1;
    if (e == hipSuccess) {
        const int nt = (many + KT_TILE - 1) / KT_TILE;
        hipLaunchKernelGGL(g2g_msa_div_kernel, dim3(nt, nt), dim3(KT_TILE * KT_TILE), 0, ctx->stream, d_codes, many, len,
                           (double *) (dev + o_pdist), (int *) (dev + o_pcnt));
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        const size_t lanes = (size_t) len * num;
        hipLaunchKernelGGL(g2g_grp_cols_kernel, dim3((unsigned) ((lanes + KG_THREADS - 1) / KG_THREADS)), dim3(KG_THREADS), 0, ctx->stream,
                           d_codes, many, len, num, d_gstart, (unsigned short *) (dev + o_res), (unsigned short *) (dev + o_R));
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(g2g_grp_gap_kernel, dim3((many + KG_THREADS - 1) / KG_THREADS, num), dim3(KG_THREADS), 0, ctx->stream,
                           d_codes, many, len, num, d_gstart, d_grp, (const unsigned short *) (dev + o_res), (const unsigned short *) (dev + o_R),
                           (int *) (dev + o_part));
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(g2g_grp_reduce_kernel, dim3(num, num), dim3(64), 0, ctx->stream, (const int *) (dev + o_pcnt), (const int *) (dev + o_part),
                           d_gstart, many, (double *) (dev + o_dist), (int *) (dev + o_cnt));
        e = hipGetLastError();
    }
    if (e == hipSuccess && timed) e = hipEventRecord(ctx->ev[1], ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dist, dev + o_dist, 8 * npg, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && counts) e = hipMemcpyAsync(counts, dev + o_cnt, 16 * npg, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && slot_dist) e = hipMemcpyAsync(slot_dist, dev + o_pdist, 8 * npm, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess && timed) e = g2g_note_events(ctx, "KTREE_GROUPS_KERNEL_MS", ctx->ev[0], ctx->ev[1], false);   // (g2g_get_option reads it)
    (void) hipFree(dev);
    if (e != hipSuccess) { g2g_errorf(who, "%s", hipGetErrorString(e)); (void) hipGetLastError(); return G2G_ERR_DEVICE; }
    return G2G_OK;
}

static int kg_check_args(const char *who, int many, int len, const uint8_t *codes, const g2g_subset *groups)
{
    if (!codes || !groups) { g2g_set_error("%s: bad argument", who); return G2G_ERR_ARG; }
    if (many < 2 || many > G2G_KTREE_MAX_MEMBERS || len < 1) { g2g_set_error("%s: 2 <= many <= 4096 and len >= 1", who); return G2G_ERR_ARG; }
    return kg_check_groups(who, many, len, groups);
}

extern "C" int g2g_msa_divergence_groups(g2g_ctx *ctx, int many, int len, const uint8_t *codes, const g2g_subset *groups,
                                         double *dist, int32_t *counts)
{
    const char *who = "g2g_msa_divergence_groups";
    if (!dist) { g2g_set_error("%s", "g2g_msa_divergence_groups: bad argument"); return G2G_ERR_ARG; }
    const int rc = kg_check_args(who, many, len, codes, groups);
    if (rc != G2G_OK) return rc;
    if (!ctx || !ctx->ok) { g2g_set_error("%s", "g2g_msa_divergence_groups: no device (there is no CPU path)"); return G2G_ERR_NODEVICE; }
    return kg_divergence(who, ctx, many, len, codes, groups, dist, counts, NULL);
}

extern "C" int g2g_ktree_from_dist_leaves(int num, const double *dist, const int32_t *ndesc, const double *height, const double *res,
                                          int with_weights, g2g_ktree *out)
{
    if (!dist || !out || num < 2 || num > G2G_KTREE_MAX_MEMBERS) { g2g_set_error("%s", "g2g_ktree_from_dist_leaves: bad argument (2 <= num <= 4096)"); return G2G_ERR_ARG; }
    return kt_tree_from_dist("g2g_ktree_from_dist_leaves", num, dist, ndesc, height, res, with_weights, out);
}

// Knode::kirchhof from the root (src/phyl.cc:637-649) over a tree of g2g_ktree_from_dist: vol is the potential of a node, cur the
// current through the branch above it.  Fathers are made after their sons: descending node ids visit a father first.
static void kg_kirchhof(const g2g_ktree &t, std::vector<double> &vol, std::vector<double> &cur)
{
    vol.assign(t.n_nodes, 0.); cur.assign(t.n_nodes, 0.);
    for (int k = t.n_nodes; k-- > 0; ) {
        const int par = t.parent[k];
        if (par < 0) { vol[k] = t.res[k]; cur[k] = 1.; continue; }
        const double pres = t.res[k] + t.length[k];
        cur[k] = pres > 0. ? vol[par] / pres : cur[par] / 2.;
        vol[k] = vol[par] - t.length[k] * cur[k];
    }
}

extern "C" int g2g_ktree_from_msa_groups(g2g_ctx *ctx, int many, int len, const uint8_t *codes, const g2g_subset *groups, int flat_leaves,
                                         g2g_ktree *out, double *weight, double *sumwt)
{
    const char *who = "g2g_ktree_from_msa_groups";
    if (!out || !weight) { g2g_set_error("%s", "g2g_ktree_from_msa_groups: bad argument"); return G2G_ERR_ARG; }
    int rc = kg_check_args(who, many, len, codes, groups);
    if (rc != G2G_OK) return rc;
    if (!ctx || !ctx->ok) { g2g_set_error("%s", "g2g_ktree_from_msa_groups: no device (there is no CPU path)"); return G2G_ERR_NODEVICE; }
    const int num = groups->num;
    std::vector<double> gdist((size_t) num * (num - 1) / 2), sdist((size_t) many * (many - 1) / 2);
    rc = kg_divergence(who, ctx, many, len, codes, groups, gdist.data(), NULL, sdist.data());
    if (rc != G2G_OK) return rc;
    std::vector<int32_t> ndesc(num);
    std::vector<double> height(num, 0.), res(num, 0.), sub, vol, cur;
    for (int g = 0; g < num; ++g) {                                   // prrn5.cc:348-372
        const int s = groups->start[g], n = groups->start[g + 1] - s;
        ndesc[g] = n;
        if (n == 1) { weight[groups->member[s]] = 1.; continue; }
        sub.resize((size_t) n * (n - 1) / 2);
        for (int j = 1; j < n; ++j)
            for (int i = 0; i < j; ++i) sub[kt_elem(i, j)] = sdist[kt_elem(s + i, s + j)];
        g2g_ktree t;
        rc = kt_tree_from_dist(who, n, sub.data(), NULL, NULL, NULL, 0, &t);
        if (rc != G2G_OK) return rc;
        kg_kirchhof(t, vol, cur);
        for (int i = 0; i < n; ++i) weight[groups->member[s + i]] = (t.ndesc[t.root] * cur[i] + t.ndesc[i] * 0.) * (1. / (1. + 0.));   // calcwt, F_UNIF_WEIGHT = 0
        if (!flat_leaves) { height[g] = t.height[t.root]; res[g] = t.res[t.root]; }
        g2g_ktree_free(&t);
    }
    rc = kt_tree_from_dist(who, num, gdist.data(), ndesc.data(), height.data(), res.data(), 1, out);
    if (rc != G2G_OK) return rc;
    for (int g = 0; g < num; ++g)
        for (int k = groups->start[g]; k < groups->start[g + 1]; ++k) weight[groups->member[k]] *= out->vol[g];
    if (sumwt) {
        double s = 0;
        for (int m = 0; m < many; ++m) s += weight[m];
        *sumwt = s;
    }
    return G2G_OK;
}
