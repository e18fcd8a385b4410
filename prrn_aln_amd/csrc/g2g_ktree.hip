// g2g_ktree.hip -- the weighting tree of an MSA: Ssrel::calcweight -> Ktree(msd) -> calcpw (reference src/prrn5.cc:385-386).
// Three steps, each the reference's own arithmetic (IEEE doubles, its operation order, no contraction), so the tree -- topology,
// heights, Kirchhoff vol / cur -- is the reference's bit for bit (tests/test_ktree_host.py, tests/test_gpu_ktree.py):
//   1. the pairwise divergence of all members, calcdistseq / pairdvn (src/phyl.cc:344-385, src/divseq.cc:33-63): many (many - 1) / 2
//      walks over the columns -- the data-parallel part, g2g_msa_div_kernel below
//   2. DistTree::upg_method with its nearest-neighbour cache (src/phyl.cc:911-1026) and Knode::teachparent (:583-595)
//   3. Ktree::calcpw -> pairwt (src/phyl.cc:704-767, 813-826): the Kirchhoff weights
// 2 and 3 are small serial host work (O(many^2) in practice) and need no device.
//
// Kernel mapping: ONE WORKGROUP PER 16 x 16 TILE OF PAIRS, one lane per pair (i = tile row + lane % 16, j = tile column + lane / 16;
// tiles below the diagonal leave at once, the lanes of a diagonal tile with i >= j are masked at the store).  The walk of a pair is
// a serial recurrence over the columns (two gap-run counters decide whether an unpaired column opens a gap), so the columns are
// not split: the workgroup goes through them in chunks of KT_CHUNK, staging the two 16-member slabs of a chunk in LDS --
// TRANSPOSED, [member][column], so that a lane fetches 16 columns of its member with one ds_read_b128 -- and every lane carries
// its six counters in registers from chunk to chunk.  Rows are KT_CHUNK + 16 bytes apart: the 16 rows a lane group reads start in
// 16 different 16-byte slots of the 256-byte bank row (no conflict; lanes on the same row read the same address).
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>

#define KT_TILE 16
#define KT_CHUNK 256
#define KT_ROW (KT_CHUNK + 16)

struct KtCount { int mch, mmc, unp, gap, gsi, gsj; };
// one column of pairdvn (divseq.cc:40-60); a code <= 1 is a gap (IsGap: nil 0 and gap 1).  Note the asymmetry of the reference:
// on a gap / gap column gsi advances and gsj stands still.
// Written on all-ones / zero masks in ordinary integers, not on bools: sixteen columns' worth of comparison results would
// otherwise live in scalar register pairs (one 64-lane mask each) and spill.
__host__ __device__ __forceinline__ void kt_column(KtCount &c, const int a, const int b)
{
    const int ga = (a - 2) >> 31, gb = (b - 2) >> 31;                 // -1: a gap
    const int one = ga ^ gb, both = ~(ga | gb);
    const int eq = ((a ^ b) - 1) >> 31;                               // -1: a == b (codes are 0 .. 255)
    const int d = c.gsj - c.gsi;
    const int sd = (d ^ ~ga) - ~ga;                                   // ga ? gsj - gsi : gsi - gsj
    c.unp -= one;
    c.gap -= one & ~(sd >> 31);                                       // ga ? gsi <= gsj : gsi >= gsj
    c.mch -= both & eq;
    c.mmc -= both & ~eq;
    c.gsj = (c.gsj - (gb & ~ga)) & gb;                                // gb ? (ga ? gsj : gsj + 1) : 0
    c.gsi = (c.gsi + 1) & ga;                                         // ga ? gsi + 1 : 0
}
// divseq.cc:61-62 (gapfrac = 0.8, a variable there: 1 - gapfrac is the double difference, not 0.2)
__host__ __device__ __forceinline__ double kt_dist(const KtCount &c)
{
    const double gapfrac = 0.8;
    const double gapunp = gapfrac * c.gap + (1 - gapfrac) * c.unp;
    return 1. - (double) c.mch / (gapunp + c.mch + c.mmc);
}

extern "C" __global__ void __launch_bounds__(KT_TILE * KT_TILE) g2g_msa_div_kernel(const uint8_t *codes, const int many, const int len,
                                                                                  double *dist, int *counts)
{
    if (blockIdx.x > blockIdx.y) return;                             // (tile row > tile column: every pair has i > j)
    __shared__ __attribute__((aligned(16))) unsigned char slab[2][KT_TILE][KT_ROW];
    const int tid = threadIdx.x, x = tid & (KT_TILE - 1), y = tid >> 4;
    const int i0 = blockIdx.x * KT_TILE, j0 = blockIdx.y * KT_TILE;
    KtCount c = {0, 0, 0, 0, 0, 0};
    for (int c0 = 0; c0 < len; c0 += KT_CHUNK) {
        const int n = min(KT_CHUNK, len - c0);
        // stage: 16 consecutive threads take the 16 members of one column (consecutive bytes of the MSA); members past the end
        // read as gaps and belong to masked lanes only
        for (int k = tid; k < n * KT_TILE; k += KT_TILE * KT_TILE) {
            const int col = k >> 4, m = k & (KT_TILE - 1);
            const size_t at = (size_t) (c0 + col) * many;
            slab[0][m][col] = i0 + m < many ? codes[at + i0 + m] : 1;
            slab[1][m][col] = j0 + m < many ? codes[at + j0 + m] : 1;
        }
        __syncthreads();
        int g = 0;
        for (; g + 16 <= n; g += 16) {
            const uint4 va = *(const uint4 *) &slab[0][x][g], vb = *(const uint4 *) &slab[1][y][g];
            const unsigned wa[4] = {va.x, va.y, va.z, va.w}, wb[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
            for (int k = 0; k < 16; ++k) kt_column(c, (int) ((wa[k >> 2] >> (8 * (k & 3))) & 255u), (int) ((wb[k >> 2] >> (8 * (k & 3))) & 255u));
        }
        for (; g < n; ++g) kt_column(c, slab[0][x][g], slab[1][y][g]);
        __syncthreads();
    }
    const int i = i0 + x, j = j0 + y;
    if (i < j && j < many) {
        const size_t k = (size_t) j * (j - 1) / 2 + i;                // elem(i, j), cmn.h:115-117
        dist[k] = kt_dist(c);
        int4 o; o.x = c.mch; o.y = c.mmc; o.z = c.unp; o.w = c.gap;
        *(int4 *) (counts + 4 * k) = o;
    }
}

#define G2G_KTREE_MAX_MEMBERS 4096

extern "C" int g2g_msa_divergence(g2g_ctx *ctx, int many, int len, const uint8_t *codes, double *dist, int32_t *counts)
{
    if (!ctx || !codes || !dist) { g2g_set_error("%s", "g2g_msa_divergence: bad argument"); return G2G_ERR_ARG; }
    if (many < 2 || many > G2G_KTREE_MAX_MEMBERS || len < 1) { g2g_set_error("%s", "g2g_msa_divergence: 2 <= many <= 4096 and len >= 1"); return G2G_ERR_ARG; }
    if (!ctx->ok) return G2G_ERR_NODEVICE;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t np = (size_t) many * (many - 1) / 2, nb = (size_t) many * len;
    auto al = [](size_t v) { return (v + 255) & ~(size_t) 255; };
    const size_t o_dist = al(nb), o_cnt = al(o_dist + 8 * np), total = o_cnt + 16 * np;
    char *dev = 0;
    HIPCHK(hipMalloc((void **) &dev, total));
    hipError_t e = hipMemcpyAsync(dev, codes, nb, hipMemcpyHostToDevice, ctx->stream);
    const bool timed = g2g_opt(ctx, "KTREE_TIMING") != 0;            // diagnostic switch: device events around the kernel (tools/ktree_probe.py)
    if (e == hipSuccess && timed) e = hipEventRecord(ctx->ev[0], ctx->stream);
    if (e == hipSuccess) {
        const int nt = (many + KT_TILE - 1) / KT_TILE;
        hipLaunchKernelGGL(g2g_msa_div_kernel, dim3(nt, nt), dim3(KT_TILE * KT_TILE), 0, ctx->stream, (const uint8_t *) dev, many, len,
                           (double *) (dev + o_dist), (int *) (dev + o_cnt));
        e = hipGetLastError();
    }
    if (e == hipSuccess && timed) e = hipEventRecord(ctx->ev[1], ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dist, dev + o_dist, 8 * np, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && counts) e = hipMemcpyAsync(counts, dev + o_cnt, 16 * np, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess && timed) e = g2g_note_events(ctx, "KTREE_KERNEL_MS", ctx->ev[0], ctx->ev[1], false);   // (g2g_get_option reads it)
    (void) hipFree(dev);
    if (e != hipSuccess) { g2g_set_error("g2g_msa_divergence: %s", hipGetErrorString(e)); (void) hipGetLastError(); return G2G_ERR_DEVICE; }
    return G2G_OK;
}

// ---- host: the tree ------------------------------------------------------------------------------------------------------
namespace {
struct KtNode { int left, right, parent, ndesc; double height, length, res, vol, cur, ros; };
const double kt_epsilon = 1.e-7;                                      // fepsilon, cmn.h:54
inline size_t kt_elem(int i, int j) { return i < j ? (size_t) j * (j - 1) / 2 + i : (size_t) i * (i - 1) / 2 + j; }   // cmn.h:115-117

struct KtBuilder {
    int many;
    const int32_t *leaf_ndesc = 0;                                    // what IterMsa::phyl_pwt puts into lead[k] before Ktree(msd, ss, UPG_METHOD, lead)
    const double *leaf_height = 0, *leaf_res = 0;                     // (src/prrn5.cc:364-371): leaves that are sub-alignments; NULL: 1 / 0 / 0
    std::vector<double> dist;                                         // the working copy: upg_method averages in place
    std::vector<KtNode> lead;
    std::vector<int> row, nnbr, nodes;
    double &distance(int i, int j) { return dist[kt_elem(i, j)]; }    // phyl.h:461

    // DistTree::dminidx, phyl.cc:911-925: the row whose cached nearest neighbour is closest; the first minimum wins
    double dminidx(int &ii, int members)
    {
        ii = row[0];
        double dmin = distance(ii, nnbr[ii]);
        for (int j = 0; ++j < members; ) {
            const int jj = row[j];
            const double dij = distance(jj, nnbr[jj]);
            if (dij < dmin) { ii = jj; dmin = dij; }
        }
        return dmin;
    }
    // DistTree::dminrow, phyl.cc:927-941: the nearest neighbour of ii among the live rows; ii itself when there is none
    int dminrow(int ii, int members)
    {
        double dmin = FLT_MAX;
        int jj = ii;
        for (int k = 0; k < members; ++k) {
            const int kk = row[k];
            if (kk == ii) continue;
            const double dij = distance(ii, kk);
            if (dij < dmin) { dmin = dij; jj = kk; }
        }
        return jj;
    }
    // DistTree::upg_method, phyl.cc:943-1026, treemode.method = UPG_METHOD; returns the root
    int upg_method()
    {
        const int members = many;
        lead.assign((size_t) 2 * members - 1, KtNode{-1, -1, -1, 0, 0., 0., 0., 0., 0., 0.});
        row.resize(members); nnbr.assign(members, 0); nodes.resize(members);
        nnbr[0] = 1;
        int m = 0;
        for (size_t k = 0; m < members; ++m) {
            nodes[m] = row[m] = m;
            lead[m].ndesc = leaf_ndesc ? std::max(leaf_ndesc[m], 1) : 1;   // phyl.cc:956
            if (leaf_height) lead[m].height = leaf_height[m];
            if (leaf_res) lead[m].res = leaf_res[m];
            for (int n = 0; n < m; ++n, ++k) {
                if (dist[k] < distance(m, nnbr[m])) nnbr[m] = n;
                if (dist[k] < distance(n, nnbr[n])) nnbr[n] = m;
            }
        }
        int root = 0;
        for (int n = members; n-- > 1; ) {
            int ii = 0;
            const double dij = dminidx(ii, n);                         // (n + 1 rows are live: the reference leaves the last one out of this scan)
            const int jj = nnbr[ii];
            root = m++;
            KtNode &rt = lead[root];
            const int ln = rt.left = nodes[ii], rn = rt.right = nodes[jj];
            KtNode &lnode = lead[ln], &rnode = lead[rn];
            rt.height = dij / 2;
            lnode.length = rt.height - lnode.height;
            if (lnode.length < 0) lnode.length = 0;
            rnode.length = rt.height - rnode.height;
            if (rnode.length < 0) rnode.length = 0;
            const double rl = lnode.res + rt.height - lnode.height;
            const double rr = rnode.res + rt.height - rnode.height;
            rt.res = (rl > kt_epsilon && rr > kt_epsilon) ? (rl * rr) / (rl + rr) : kt_epsilon;
            rt.ndesc = lnode.ndesc + rnode.ndesc;
            int j = 0;
            for (int k = 0; k <= n; ++k) {
                nnbr[ii] = -1;
                const int kk = row[k];
                if (kk == ii) continue;
                if (kk == jj) { j = k; continue; }
                double &x = distance(kk, ii);
                const double y = distance(kk, jj);
                x *= lnode.ndesc;                                     // three roundings, as the reference's three statements
                x += rnode.ndesc * y;
                x /= rt.ndesc;
                if (nnbr[kk] == ii || nnbr[kk] == jj) nnbr[kk] = -1;  // its neighbour is gone: look again below
            }
            nodes[ii] = root;
            row[j] = row[n];
            for (int k = 0; k < n; ++k) {
                const int kk = row[k];
                if (nnbr[kk] < 0) nnbr[kk] = dminrow(kk, n);
            }
        }
        teachparent(root);
        lead[root].parent = -1;
        return root;
    }
    // Knode::teachparent, phyl.cc:583-595: parents, ndesc, and the subtree with the smaller lowest leaf goes left
    int teachparent(int id)
    {
        KtNode &nd = lead[id];
        if (nd.left < 0) return id;
        lead[nd.left].parent = lead[nd.right].parent = id;
        int l = teachparent(nd.left);
        const int r = teachparent(nd.right);
        nd.ndesc = lead[nd.left].ndesc + lead[nd.right].ndesc;
        if (l > r) { l = r; std::swap(nd.left, nd.right); }
        return l;
    }
    // Ktree::pairwt, phyl.cc:704-767, with wfact = 0 / cfact = true (phyl.cc:77-78); the pair-weight table is not formed here
    void pairwt(int id, double ros, int root)
    {
        KtNode &node = lead[id];
        node.ros = ros;
        if (node.left < 0) { node.vol = lead[node.parent].vol * node.cur; return; }
        KtNode &left = lead[node.left], &right = lead[node.right];
        double a = left.res + left.length;
        double b = right.res + right.length;
        if (id == root) {
            node.cur = left.cur = right.cur = 1;
        } else if (node.ros <= kt_epsilon || a + b <= kt_epsilon) {
            a = b = 0;
            left.cur = right.cur = 0.5;
            node.vol = node.cur * lead[node.parent].vol;
        } else {
            if (a <= 0.) { b += a; a = kt_epsilon; }
            if (b <= 0.) { a += b; b = kt_epsilon; }
            const double c = node.length + node.ros;
            double wab = a * b / (a + b);
            double wbc = a * (b + c);
            const double wfa = 1. + a * node.ros / ((wab + c) * (a + c));
            const double wfb = 1. + b * node.ros / ((wab + c) * (b + c));
            wab = wbc + b * c;
            wbc /= wab * wfb;
            const double wac = b * (a + c) / (wab * wfa);
            wab = c * (a + b) / wab;
            a *= node.ros / (a + node.ros);
            b *= node.ros / (b + node.ros);
            node.cur *= sqrt(wac * wbc / wab);
            node.vol = node.cur * lead[node.parent].vol;
            left.cur = sqrt(wab * wac / wbc);
            right.cur = sqrt(wab * wbc / wac);
        }
        pairwt(node.left, b, root);
        pairwt(node.right, a, root);
    }
};
}

extern "C" void g2g_ktree_free(g2g_ktree *t)
{
    if (!t) return;
    free(t->left); free(t->right); free(t->parent); free(t->ndesc);
    free(t->height); free(t->length); free(t->res); free(t->vol); free(t->cur);
    memset(t, 0, sizeof *t);
}

// the builder behind g2g_ktree_from_dist and g2g_ktree_from_dist_leaves (include/g2g_groups.h): num leaves, preset or plain
static int kt_tree_from_dist(const char *who, int many, const double *dist, const int32_t *ndesc, const double *height, const double *res,
                             int with_weights, g2g_ktree *out)
{
    const size_t np = (size_t) many * (many - 1) / 2;
    for (int j = 1; j < many; ++j)
        for (int i = 0; i < j; ++i) {
            const double d = dist[kt_elem(i, j)];
            if (!(d >= 0)) {                                          // (NaN included: a pair of members without a common column)
                g2g_errorf(who, "distance of members %d and %d is %s", i, j, d != d ? "not a number" : "negative");
                return G2G_ERR_ARG;
            }
        }
    KtBuilder B;
    B.many = many;
    B.leaf_ndesc = ndesc; B.leaf_height = height; B.leaf_res = res;
    B.dist.assign(dist, dist + np);
    const int root = B.upg_method();
    if (with_weights) {                                               // Ktree::calcpw, phyl.cc:813-826
        B.lead[root].vol = 1.;
        B.pairwt(root, FLT_MAX, root);                                // fInfinit, cmn.h:55
    }
    const int nn = 2 * many - 1;
    memset(out, 0, sizeof *out);
    out->left = (int32_t *) malloc(4 * (size_t) nn); out->right = (int32_t *) malloc(4 * (size_t) nn);
    out->parent = (int32_t *) malloc(4 * (size_t) nn); out->ndesc = (int32_t *) malloc(4 * (size_t) nn);
    out->height = (double *) malloc(8 * (size_t) nn); out->length = (double *) malloc(8 * (size_t) nn); out->res = (double *) malloc(8 * (size_t) nn);
    out->vol = (double *) malloc(8 * (size_t) nn); out->cur = (double *) malloc(8 * (size_t) nn);
    if (!out->left || !out->right || !out->parent || !out->ndesc || !out->height || !out->length || !out->res || !out->vol || !out->cur) {
        g2g_ktree_free(out);
        return G2G_ERR_NOMEM;
    }
    out->n_nodes = nn; out->root = root;
    for (int k = 0; k < nn; ++k) {
        const KtNode &nd = B.lead[k];
        out->left[k] = nd.left; out->right[k] = nd.right; out->parent[k] = nd.parent; out->ndesc[k] = nd.ndesc;
        out->height[k] = nd.height; out->length[k] = nd.length; out->res[k] = nd.res;
        out->vol[k] = with_weights ? nd.vol : 0.; out->cur[k] = with_weights ? nd.cur : 0.;
    }
    return G2G_OK;
}

extern "C" int g2g_ktree_from_dist(int many, const double *dist, int with_weights, g2g_ktree *out)
{
    if (!dist || !out || many < 2 || many > G2G_KTREE_MAX_MEMBERS) { g2g_set_error("%s", "g2g_ktree_from_dist: bad argument (2 <= many <= 4096)"); return G2G_ERR_ARG; }
    return kt_tree_from_dist("g2g_ktree_from_dist", many, dist, NULL, NULL, NULL, with_weights, out);
}

extern "C" int g2g_ktree_from_msa(g2g_ctx *ctx, int many, int len, const uint8_t *codes, g2g_ktree *out)
{
    if (!out) { g2g_set_error("%s", "g2g_ktree_from_msa: bad argument"); return G2G_ERR_ARG; }
    if (many < 2 || many > G2G_KTREE_MAX_MEMBERS) { g2g_set_error("%s", "g2g_ktree_from_msa: 2 <= many <= 4096"); return G2G_ERR_ARG; }
    std::vector<double> dist((size_t) many * (many - 1) / 2);
    const int rc = g2g_msa_divergence(ctx, many, len, codes, dist.data(), NULL);
    return rc != G2G_OK ? rc : g2g_ktree_from_dist(many, dist.data(), 1, out);
}
