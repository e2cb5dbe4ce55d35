/* densecap_debug_optim.h -- test hooks of the optimiser's kernels (optim.hip).
 *
 * Like densecap_debug.h, NOT part of the drop-in boundary: tests/ and tools/ use them to run a kernel alone, through its
 * production launcher.  They live in a header of their own because the lists of hooks in the other debug headers are pinned by
 * tests.  Device pointers unless stated; every hook synchronises before it returns.  No weights needed.
 */
#ifndef DENSECAP_DEBUG_OPTIM_H
#define DENSECAP_DEBUG_OPTIM_H

#include "densecap.h"

#ifdef __cplusplus
extern "C" {
#endif

/* dc_op_adam over nseg segments in ONE launch, as dc_train_step issues it: HOST arrays of nseg DEVICE pointers p, g, m, v and
 * of nseg lengths n (each >= 1); 1 <= nseg <= 4096.  grid = 0: the production grid; > 0: that many workgroups (the result does
 * not depend on it). */
int dc_debug_adam_multi(dc_ctx* ctx, float* const* p, const float* const* g, float* const* m, float* const* v, const size_t* n,
                        int nseg, int t, const dc_train_opts* opts, int grid);
/* The decode screen's operands as dc_train_step remakes them: W (V1, Hd) fp32 -> wb (V1pad, Kp) bf16 bits (round to nearest
 * even, zero padding) and wn (V1pad) fp16 bits, every row's 2-norm rounded up (zero past V1).  V1pad >= V1, Kp >= Hd. */
int dc_debug_screen_operands(dc_ctx* ctx, const float* W, int V1, int Hd, int V1pad, int Kp, uint16_t* wb, uint16_t* wn);
/* dc_op_pack_conv3x3_weights' inverse, as dc_get_weights uses it: (Cout, 9 Cin) packed -> OIHW. */
int dc_debug_unpack_conv3x3(dc_ctx* ctx, const float* w_packed, float* w_oihw, int Cout, int Cin);

#ifdef __cplusplus
}
#endif
#endif /* DENSECAP_DEBUG_OPTIM_H */
