/* densecap_debug_clip.h -- test hook of gradient clipping (optim.hip; docs/SEMANTICS.md, "Gradient clipping").
 *
 * Like densecap_debug_optim.h, NOT part of the drop-in boundary, and in a header of its own because the lists of hooks in the
 * other debug headers are pinned by tests.  Device pointers unless stated; the hook synchronises before it returns.  No weights
 * needed.
 */
#ifndef DENSECAP_DEBUG_CLIP_H
#define DENSECAP_DEBUG_CLIP_H

#include "densecap.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The sequence dc_train_step issues with clipping on, over nseg caller-supplied segments (the lists of dc_debug_adam_multi): the
 * two norm kernels over all the g, then the scaled Adam launch.  grid = 0: the production grids; > 0: that many workgroups in
 * both multi-workgroup launches (no result depends on it).  max_norm as dc_train_set_grad_clip takes it (0: scale = 1).
 * sumsq, scale: HOST pointers, either may be null. */
int dc_debug_adam_multi_clip(dc_ctx* ctx, float* const* p, const float* const* g, float* const* m, float* const* v, const size_t* n,
                             int nseg, int t, const dc_train_opts* opts, int grid, double max_norm, double* sumsq, float* scale);

#ifdef __cplusplus
}
#endif
#endif /* DENSECAP_DEBUG_CLIP_H */
