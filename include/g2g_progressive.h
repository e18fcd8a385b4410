/*
 * g2g_progressive.h -- C ABI of libg2g.so, continued: the progressive alignment over a guide tree.
 *
 * A header of its own beside g2g.h, which it includes: g2g.h is read by every device translation unit of the library, and these
 * entry points are host code over level 1 of that ABI -- they add nothing a kernel sees.  (Entry points added without a change of
 * g2g_abi_version.)
 *
 * <-> ProgMsa<node_t>::prog_up (reference src/prrn5.h:85-105), the step of makemsa between the guide tree (Ktree(&dm),
 * src/prrn5.cc:978-979 <-> g2g_ktree_from_dist(with_weights = 0)) and the first MSA: post-order over the tree, and at every inner
 * node  exg_seq(0, 0)  of both sons' results and  mSeq* align2(mSeq** sqs, 0, alnprm)  (src/maln2.cc:2048-2061) = PwdM(sqs), which
 * may swap the two (selAlnMode, :81-154), align2(sqs, &pwd, ...) (:1875), and syntheseq (:2027-2046: skl2gaps + unfoldgap +
 * aggregate(sd, sqs, gps, 0), src/mgaps.cc:282-341) on the SWAPPED order -- the members of the PwdM's `a` side come first in the
 * merged MSA, then those of `b`.  wtlst is 0: a merged group carries no weights, every merge is an unweighted PwdM.
 *
 * Here the tree is walked in WAVES of independent merges: a wave is every node whose two sons are done, in ascending node id, at
 * most max_batch of them at a time.  Both sons of a node become groups (g2g_group_create, weight = NULL), the PwdMs of a wave are
 * built by one g2g_pwdm_create_batch, its DPs run in one g2g_align2_batch (the end check and the sh = -100 retry included), and a
 * skeleton is applied by interleaving the two blocks' columns, as g2g_refine applies an accepted move.  A son's group and block
 * are released once its father is merged.  One context, no threads beyond those the builders use.  The result does not depend on
 * max_batch.
 *
 *   seqs   : nseq single sequences taken whole: left = 0 and right = len (else G2G_ERR_ARG), len >= 1.
 *   tree   : n_nodes = 2 nseq - 1, nodes 0 .. nseq - 1 are the leaves = the sequences, left / right / parent = -1 where absent.
 *            vol / cur are not read and may be NULL: the output of g2g_ktree_from_dist(.., 0, ..) is usable as it is.  The tree is
 *            validated; a malformed one is G2G_ERR_ARG and g2g_last_error names the node: not exactly one root, a leaf with sons,
 *            an inner node with one son, a node reached twice, a parent that does not agree with its father's left / right.
 *   opts   : may be NULL.  max_batch: most merges of one batch, 0 = 64.  reserved 0.
 *            aligner: takes g2g_align2_batch's seat (same arguments behind `user`; skl[i] malloc'ed, the library frees it; a
 *            nonzero return ends the call with that code).  ctx may be NULL only when it is set -- the PwdMs are then built on the
 *            host, one g2g_pwdm_create each.  The tests drive the whole walk on a machine without a GPU this way, with the CPU
 *            checker in the aligner's seat; the product never sets it.
 * Outputs:
 *   *out_codes : malloc'ed (g2g_free), *out_len x nseq residue codes [column][member], gap = 1.
 *   order      : nseq ints from the caller: order[k] = the input index of member k of the result.
 *   *merges    : malloc'ed (g2g_free; merges / nmerges may be NULL), one record per inner node in the order merged: the node and
 *                its sons, na / nb = the members of the PwdM's a / b side (after the swap), swp, mode = g2g_problem::alnmode, the
 *                wave, the merged length, the DP score and the wall clock since the call began when the wave's merges were done.
 *   stats      : may be NULL; waves = batches of DPs run, wait_timeouts / recovered_dps as in g2g_refine_stats.
 * nseq == 1 returns the sequence itself with no merge.
 * G2G_ERR_MODE, before anything is built: tgapf != 1, u0 > 0, banded != 1 (the limits of g2g_refine_planned).  A DP that comes
 * back with a nonzero status ends the call with that status: g2g_last_error names the node, everything is freed, nothing is
 * handed out.
 * Not on this path: leaves that are groups or carry weights, discounted terminal gaps (tgapf < 1: the nil codes aggregate hands
 * on), annotated sequences (exon boundaries), local ends (algmode.lcl), and the guide FOREST of SlfPrrn (SlfPrrn::make_msa, src/prrn5.cc:1174-1230).
 */
#ifndef G2G_PROGRESSIVE_H_
#define G2G_PROGRESSIVE_H_

#include "g2g.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef int (*g2g_align_fn)(void *user, int n, g2g_pwdm *const *pw, double *scr, g2g_skl **skl, int *nskl, int *status);
typedef struct g2g_prog_opts {
    int32_t max_batch, reserved;
    g2g_align_fn aligner;           /* NULL: g2g_align2_batch on the GPU */
    void   *aligner_user;
} g2g_prog_opts;
typedef struct g2g_prog_merge {
    int32_t node, left, right, na, nb, swp, mode, wave, len;
    int32_t reserved;
    double  scr, t_ms;
} g2g_prog_merge;
typedef struct g2g_prog_stats {
    int32_t merges, waves, largest_wave;
    int32_t wait_timeouts, recovered_dps, reserved;
} g2g_prog_stats;
int g2g_progressive(g2g_ctx *ctx, const g2g_params *prm, int nseq, const g2g_dseq *seqs, const g2g_tree *tree,
                    const g2g_prog_opts *opts, uint8_t **out_codes, int *out_len, int32_t *order,
                    g2g_prog_merge **merges, int *nmerges, g2g_prog_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* G2G_PROGRESSIVE_H_ */
