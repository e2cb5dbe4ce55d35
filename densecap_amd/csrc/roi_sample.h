// The sampling position of one (box, point) of bilinear RoI pooling, shared by the forward kernel (roipool.hip) and the
// backward kernels (recog_grad.hip) so that floors and weights are the same bits in both directions.
// BoxToAffine.lua:88-91 -> AffineGridGeneratorBHWD -> BilinearSamplerBHWD_updateOutput, every fp32 op rounded once in source
// order.  Include it AFTER `#pragma clang fp contract(off)`.
#ifndef DENSECAP_ROI_SAMPLE_H
#define DENSECAP_ROI_SAMPLE_H

#include "common.h"

struct RoiPoint {
  int x0, y0;      // the top-left tap (clamped to [-2, dim + 1]: anything outside [-1, dim] is invalid either way)
  float wx, wy;    // the top-left tap's weights along x and y
};

// the base grid of AffineGridGeneratorBHWD: -1 + 2 * i / (n - 1), computed in double then rounded
__device__ __forceinline__ float roi_base_coord(int i, int n) { return (float)(-1.0 + ((double)i / (double)(n - 1)) * 2.0); }

// point (i, j) of the HH x WW grid of box bx (xc, yc, w, h in image pixels) on a map of h x w pixels
__device__ __forceinline__ RoiPoint roi_point(const f32x4 bx, float img_h, float img_w, int HH, int WW, int i, int j, int h, int w) {
  // BoxToAffine.lua:88-91
  const float th23 = __fdiv_rn(__fadd_rn(__fmul_rn(bx[0], 2.f), -1.f - img_w), img_w - 1.f);
  const float th13 = __fdiv_rn(__fadd_rn(__fmul_rn(bx[1], 2.f), -1.f - img_h), img_h - 1.f);
  const float th22 = __fdiv_rn(bx[2], img_w);
  const float th11 = __fdiv_rn(bx[3], img_h);
  const float yb = roi_base_coord(i, HH);
  const float xb = roi_base_coord(j, WW);
  const float gy = __fadd_rn(__fadd_rn(__fmul_rn(yb, th11), __fmul_rn(xb, 0.f)), th13);
  const float gx = __fadd_rn(__fadd_rn(__fmul_rn(yb, 0.f), __fmul_rn(xb, th22)), th23);
  // BilinearSamplerBHWD_updateOutput
  const float xcoord = __fdiv_rn(__fmul_rn(__fadd_rn(gx, 1.f), (float)(w - 1)), 2.f);
  const float ycoord = __fdiv_rn(__fmul_rn(__fadd_rn(gy, 1.f), (float)(h - 1)), 2.f);
  const float xfl = floorf(xcoord), yfl = floorf(ycoord);
  RoiPoint r;
  // clamp before the int cast (far-away boxes)
  r.x0 = (int)fminf(fmaxf(xfl, -2.f), (float)w + 1.f);
  r.y0 = (int)fminf(fmaxf(yfl, -2.f), (float)h + 1.f);
  r.wx = __fsub_rn(1.f, __fsub_rn(xcoord, xfl));
  r.wy = __fsub_rn(1.f, __fsub_rn(ycoord, yfl));
  return r;
}

// the four blend weights in tap order tl, tr, bl, br
__device__ __forceinline__ void roi_tap_weights(float wx, float wy, float (&wt)[4]) {
  wt[0] = __fmul_rn(wx, wy);
  wt[1] = __fmul_rn(__fsub_rn(1.f, wx), wy);
  wt[2] = __fmul_rn(wx, __fsub_rn(1.f, wy));
  wt[3] = __fmul_rn(__fsub_rn(1.f, wx), __fsub_rn(1.f, wy));
}

// the four taps' pixel indices y * w + x in the same order, -1 for a tap outside the map
__device__ __forceinline__ void roi_tap_pixels(int x0, int y0, int h, int w, int (&pix)[4]) {
  const bool xin0 = x0 >= 0 && x0 <= w - 1, xin1 = x0 + 1 >= 0 && x0 + 1 <= w - 1;
  const bool yin0 = y0 >= 0 && y0 <= h - 1, yin1 = y0 + 1 >= 0 && y0 + 1 <= h - 1;
  pix[0] = (xin0 && yin0) ? y0 * w + x0 : -1;
  pix[1] = (xin1 && yin0) ? y0 * w + x0 + 1 : -1;
  pix[2] = (xin0 && yin1) ? (y0 + 1) * w + x0 : -1;
  pix[3] = (xin1 && yin1) ? (y0 + 1) * w + x0 + 1 : -1;
}

#endif  // DENSECAP_ROI_SAMPLE_H
