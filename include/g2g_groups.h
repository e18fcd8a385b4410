/*
 * g2g_groups.h -- C ABI of libg2g.so, continued: the weighting tree over groups the caller brings.
 *
 * A header of its own beside g2g.h, which it includes: g2g.h is read by every device translation unit of the library, and these
 * entry points leave those as they are.  (Entry points added without a change of g2g_abi_version.)
 *
 * <-> IterMsa::phyl_pwt in the branch ss->num < ss->elms (reference src/prrn5.cc:333-391): the members of an MSA come in groups
 * (sub-alignments that stay as they are), a weighting tree is built over the GROUPS -- Ktree(msd, ss, UPG_METHOD, lead) -- from the
 * group form of pairdvn (src/divseq.cc:65-105, reached through calcdistseq(sd, ss), src/phyl.cc:344-385), its leaves carry their
 * sub-alignment's member count, height and resistance, and a member's weight is its weight inside its group (Ktree(group).calcwt,
 * src/phyl.cc:637-649, 692-702) times the vol of the group's leaf.
 *
 * The group divergence of groups A = group[k] and B = group[l], k < l: two counter arrays gsi[ni], gsj[nj], zero at the start;
 * for every column, for every i of A in list order (outer) and every j of B in list order (inner), the pairwise rule of pairdvn
 * on (A[i], B[j]) with gsi[i] and gsj[j].  gsi[i] is shared by all j and gsj[j] by all i, and both change between the inner
 * iterations of one column: the walk is not the pairwise walk summed, and it depends on which group is A and on the member order
 * of both lists.  mch, mmc and unp do equal the sums of the pairwise counts; gap does not.  The device code (csrc/
 * g2g_ktree_groups.hip) uses a closed form of the gap count that needs no ni x nj loop; tests/ktreegrouplib.py states both forms and
 * tests/test_ktree_groups_host.py holds one to the other.
 *
 *   codes  : len x many residue codes [column][member], as for g2g_msa_divergence; a code <= 1 is a gap (nil 0 counts as one).
 *   groups : partitions the members 0 .. many - 1; every group has a member.  The member order inside a group is the caller's and
 *            is significant.
 *   dist   : one double per group pair k < l at l (l - 1) / 2 + k, formed from the four counts by the expression of
 *            g2g_msa_divergence; a pair without any counted column gives what IEEE gives (NaN).
 *   counts : 4 int32 per pair (mch, mmc, unp, gap), same order; may be NULL.
 * With every group a singleton the result is that of g2g_msa_divergence on the members in the groups' order, bit for bit.
 * Limits: 2 <= groups->num, many <= 4096, len >= 1.  The reference's counters are ints: a pair with len x ni x nj >= 2^31 is
 * refused (G2G_ERR_ARG, g2g_last_error names the pair), as is a subset that does not partition the members.  Without a usable
 * context: G2G_ERR_NODEVICE -- there is no CPU path.  Context option KTREE_TIMING leaves KTREE_GROUPS_KERNEL_MS: device time of
 * the kernels of the call.
 *
 * Not in this change: progressive merging with group leaves and distances between unaligned groups; recycle > 1; pairsum_ss /
 * recalcpw over a relation with subsets; groups that bring their own weights; tgapf != 1 and u0 > 0; any change to an existing
 * kernel.
 */
#ifndef G2G_GROUPS_H_
#define G2G_GROUPS_H_

#include "g2g.h"

#ifdef __cplusplus
extern "C" {
#endif

int g2g_msa_divergence_groups(g2g_ctx *ctx, int many, int len, const uint8_t *codes, const g2g_subset *groups,
                              double *dist, int32_t *counts);

/* DistTree::upg_method + Ktree::calcpw as g2g_ktree_from_dist restates them (the two entries share the builder), from leaves
   that start with the given ndesc (max(ndesc, 1) is kept), height and res -- what phyl_pwt puts into lead[k].  A node's length
   is clamped at 0 where a leaf is taller than its merge; the resistances rl / rr are not, and the merged res falls to fepsilon.
   NULL arrays: 1 / 0 / 0, the tree of g2g_ktree_from_dist.  num leaves, num (num - 1) / 2 distances; host only. */
int g2g_ktree_from_dist_leaves(int num, const double *dist, const int32_t *ndesc, const double *height, const double *res,
                               int with_weights, g2g_ktree *out);

/* phyl_pwt as one call, on the path where the groups bring no weights of their own (the reference's seqs != NULL: hosts).
   A group of one member has weight 1; a group of several gets Ktree(group).calcwt -- UPGMA over the divergences of its members
   (those of g2g_msa_divergence on the whole MSA with the members in list order: extseq drops no gap / gap column), Knode::kirchhof
   from the root, wt[i] = root->ndesc x cur[i] -- and its leaf the subtree's root height and res, or 0 / 0 with flat_leaves (the
   reference's `update`).  Then the tree over the groups (the two entries above, with weights) and weight[m] *= vol[leaf of m's
   group]; *sumwt is their sum in member order (may be NULL).  out is directly usable as the g2g_tree over `groups` that
   g2g_consregss and g2g_consreg_groups take.  Release out with g2g_ktree_free. */
int g2g_ktree_from_msa_groups(g2g_ctx *ctx, int many, int len, const uint8_t *codes, const g2g_subset *groups, int flat_leaves,
                              g2g_ktree *out, double *weight, double *sumwt);

/* g2g_refine_plan started from the given relation instead of singletons: consregss over `groups`, consreg(DISSIM) over the
   result, consregss per range.  tree: the tree over `groups` (2 num - 1 nodes, leaf g = group g; g2g_ktree_from_msa_groups), weight
   as that call leaves it.  The groups of every relation of the plan are unions of the given groups, each handing its members over
   in its own order; origin of plan->whole names nodes of `tree`.  Refusals as g2g_refine_plan; a subset that does not partition
   the members or a tree that is not a tree over it: G2G_ERR_ARG. */
int g2g_refine_plan_groups(g2g_ctx *ctx, const g2g_params *prm, double thr, int many, int len, const uint8_t *codes,
                           const double *weight, const g2g_tree *tree, const g2g_subset *groups, g2g_refine_plan_t *out);

/* g2g_refine_planned (the two entries share their body) with `tree` the tree over `groups` and plan == NULL meaning
   g2g_refine_plan_groups: the alignment BETWEEN the groups is refined, never the alignment inside one -- the rows of a group leave
   as they came, up to columns that are all gaps in the group.  A plan that is given is taken as it is after the validation of
   g2g_refine_planned; the relation of a range that divides a given group is G2G_ERR_ARG.  Refusals as there, and for groups /
   tree as above. */
int g2g_refine_planned_groups(g2g_ctx *ctx, const g2g_params *prm, double thr, int many, int len, const uint8_t *codes,
                              const double *weight, const g2g_tree *tree, const g2g_subset *groups, const g2g_refine_plan_t *plan,
                              const g2g_refine_opts *opts, uint8_t **out_codes, int *out_len,
                              g2g_refine_step **steps, int *nsteps, g2g_refine_range_stat **rstat, int *nrstat,
                              g2g_refine_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* G2G_GROUPS_H_ */
