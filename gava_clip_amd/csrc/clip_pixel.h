// clip_pixel.h — one pixel of the data path of video_dataset/dataset.py from decoded uint8 frames: (u8/255 - mean)/std, then
// either the evaluation branch (:117-139: bilinear short-side resize, centre crop) or the random-sample branch (:93-114 with
// auto_augment=None: a source box resized to size x size, transform.py:545-577) - torch upsample_bilinear2d,
// align_corners=False, every step in fp32 with torch's own contraction pattern.  Shared by the stand-alone preprocessing
// kernels, gava_patchify and the patch-embedding GEMM's uint8 A-tile loader, so that all of them produce the same bits.
#pragma once
#include "common.h"

// a product the compiler may NOT fuse into a following add: __fmul_rn / __fadd_rn are plain operators to hipcc (it turned
// scale * (dst + 0.5) - 0.5 into one v_fma in one kernel and not in the other), an empty asm makes the value opaque
static __device__ __forceinline__ float cp_mul(float a, float b) {
  float r = a * b;
  asm volatile("" : "+v"(r));
  return r;
}

struct ClipGeom {          // the fields of gava_clip_desc the device code reads
  const unsigned char* frames; int n_frames, height, width, t_st, rate, h_st, w_st; float scale_h, scale_w;
  int box_y, box_x, box_h, box_w, lerp4_frames; const int* frame_idx;
};

// The descriptor as the kernels use it.  The source box is clamped into the frame here (no-ops for every descriptor the host
// helpers fill - they reject such boxes): a descriptor written by hand can give wrong pixels, never an address outside
// [frames, frames + n_frames*height*width*3).
static __device__ __forceinline__ ClipGeom clip_geom(const gava_clip_desc& d) {
  ClipGeom g{d.frames, d.n_frames, d.height, d.width, d.t_st, d.rate, d.h_st, d.w_st, d.scale_h, d.scale_w,
             d.box_y, d.box_x, d.box_h, d.box_w, d.lerp4_frames, d.frame_idx};
  g.box_y = min(max(g.box_y, 0), g.height - 1); g.box_x = min(max(g.box_x, 0), g.width - 1);
  g.box_h = min(max(g.box_h, 1), g.height - g.box_y); g.box_w = min(max(g.box_w, 1), g.width - g.box_x);
  return g;
}

// source frame of output frame t: the table when there is one (random / TSN sampling, dataset.py:202-217), else the strided
// temporal crop whose tail repeats the last frame (dataset.py:163-177); clamped like the box
static __device__ __forceinline__ int clip_frame(const ClipGeom& g, int t) {
  const int f = g.frame_idx ? g.frame_idx[t] : g.t_st + t * g.rate;
  return min(max(f, 0), g.n_frames - 1);
}

// arithmetic form of output frame t (gava_clip_desc.lerp4_frames): 0 separable, 1 / 2 the four-weight kernel's vectorised
// frames / its left-over frames
static __device__ __forceinline__ int clip_form(const ClipGeom& g, int t) {
  const int T = g.lerp4_frames;
  return T <= 0 ? 0 : (t < T - T % 8 ? 1 : 2);
}

// normalised value of a byte: from the caller's table when there is one (exact, and the same bits in every kernel), else the
// two true divisions of the reference's expression
static __device__ __forceinline__ float clip_norm(const float* lut, int c, unsigned char v, float mean, float stdv) {
  return lut ? lut[c * 256 + v] : __fdiv_rn(__fsub_rn(__fdiv_rn((float)v, 255.f), mean), stdv);
}

// Output pixel (y, x) of the size x size crop of source frame f, channel c.  The first tap is clamped into the
// box as torch's guard_index_and_lambda does (never taken with a descriptor from the host helpers, whose scales keep it inside).
// Arithmetic (form 0) = torch's CPU upsample_bilinear2d (align_corners=False) bit for bit, found by trying the contraction patterns
// against the oracle (tools history, round 2): the source index is ONE fma, scale * (dst + 0.5) - 0.5, and each lerp is
// fma(w0, p0, w1 * p1) - x86 builds of torch contract exactly these.  Explicit fmaf / opaque products instead of plain
// operators: left to itself hipcc contracted the same source differently in the two kernels that use it.
// With every rounding spelled out the function can be inlined anywhere: the stand-alone preprocessing kernel and the
// patch-embedding GEMM's uint8 loader produce the same bits (tests/test_preprocess.py), and the loader's eight pixels per
// task have their 32 byte loads in flight together.
// lut: fp32 [3][256] normalised byte values, or NULL (then the reference's two true divisions with mean / stdv).
static __device__ __forceinline__ float clip_pixel1(const ClipGeom& g, const float* lut, float mean, float stdv, int f, int form,
                                                   int c, int y, int x) {
  const float sy = fmaxf(__builtin_fmaf(g.scale_h, (float)(y + g.h_st) + 0.5f, -0.5f), 0.f);
  const float sx = fmaxf(__builtin_fmaf(g.scale_w, (float)(x + g.w_st) + 0.5f, -0.5f), 0.f);
  const int y0 = min((int)sy, g.box_h - 1), x0 = min((int)sx, g.box_w - 1);
  // the neighbour of the box's last row / column is that row / column itself: the reference interpolates the CROPPED tensor
  // (transform.py:570-577); the whole-frame box of the evaluation branch gives the frame's own edge
  const int y1 = y0 + 1 < g.box_h ? y0 + 1 : g.box_h - 1;
  const int x1 = x0 + 1 < g.box_w ? x0 + 1 : g.box_w - 1;
  const float ly1 = sy - (float)y0, lx1 = sx - (float)x0;
  const float ly0 = 1.f - ly1, lx0 = 1.f - lx1;
  const unsigned char* fr = g.frames + ((size_t)f * g.height + g.box_y) * g.width * 3 + (size_t)g.box_x * 3;   // row pitch = the frame's
  const unsigned char* r0 = fr + (size_t)y0 * g.width * 3;
  const unsigned char* r1 = fr + (size_t)y1 * g.width * 3;
  const float v00 = clip_norm(lut, c, r0[x0 * 3 + c], mean, stdv), v01 = clip_norm(lut, c, r0[x1 * 3 + c], mean, stdv);
  const float v10 = clip_norm(lut, c, r1[x0 * 3 + c], mean, stdv), v11 = clip_norm(lut, c, r1[x1 * 3 + c], mean, stdv);
  if (form != 0) {
    // torch's kernel for small outputs (height + width <= 128, cpu_upsample_linear_channels_last): four rounded weight
    // products, one fma chain whose order differs between the vectorised frames and the left-over ones
    const float w00 = cp_mul(ly0, lx0), w01 = cp_mul(ly0, lx1), w10 = cp_mul(ly1, lx0), w11 = cp_mul(ly1, lx1);
    if (form == 1) return __builtin_fmaf(w00, v00, __builtin_fmaf(w01, v01, __builtin_fmaf(w11, v11, cp_mul(w10, v10))));
    return __builtin_fmaf(w11, v11, __builtin_fmaf(w10, v10, __builtin_fmaf(w00, v00, cp_mul(w01, v01))));
  }
  const float top = __builtin_fmaf(lx0, v00, cp_mul(lx1, v01)), bot = __builtin_fmaf(lx0, v10, cp_mul(lx1, v11));
  return __builtin_fmaf(ly0, top, cp_mul(ly1, bot));
}
