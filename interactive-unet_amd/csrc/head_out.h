// The output contract of every prediction head (iunet_head_fwd and the heads that promise "the output contract of iunet_head_fwd":
// the fp32 head, the split-precision head, the head in the last x2m conv's epilogue, DeepLabV3's upsampling head), written once:
// logits stored with the caller's strides; softmax; class = first maximum of the PROBABILITIES (what np.argmax over the returned
// softmax gives, predict.py:38); probs = ((accumulate ? out : 0) + p) / divisor (the 2.5-D accumulation of predict.py:101-110).
// (The softmax copies of the training kernels -- loss_terms.h and its users -- are a different trade and stay where they are.)
#pragma once
#include "common.h"

struct HeadOut {
  float* logits;       // optional, generic strides
  float* probs;        // optional, generic strides
  unsigned char* cls;  // optional, [N][vox]
  long long oN, oC, oD, oH, oW;   // output strides (elements) of logits / probs
  float divisor; int accumulate;
};

// os: the strides n, c, d, h, w, or null when neither logits nor probs is asked for
inline int head_out_fill(HeadOut& o, const char* who, void* logits, void* probs, void* cls, const long long* os, float divisor,
                         int accumulate) {
  IUNET_REQUIRE(os || (!logits && !probs), "%s: logits / probs need out_strides", who);
  o.logits = (float*)logits; o.probs = (float*)probs; o.cls = (unsigned char*)cls;
  o.oN = os ? os[0] : 0; o.oC = os ? os[1] : 0; o.oD = os ? os[2] : 0; o.oH = os ? os[3] : 0; o.oW = os ? os[4] : 0;
  o.divisor = divisor; o.accumulate = accumulate;
  return IUNET_OK;
}

// voxel v = (gz, gy, gx) of sample n, vox voxels per sample.  PRECISE: expf and a correctly rounded e / s (the fp32 and split-precision
// forms); otherwise __expf and e * (1 / s) (the 16-bit forms).
template <int NCLS, bool PRECISE>
__device__ __forceinline__ void head_store(const HeadOut& p, const float (&l)[NCLS], int n, long long vox, long long v, int gz, int gy,
                                           int gx) {
  const long long obase = n * p.oN + gz * p.oD + gy * p.oH + gx * p.oW;
  float mx = l[0];
#pragma unroll
  for (int c = 1; c < NCLS; ++c) mx = fmaxf(mx, l[c]);
  if (p.logits) {
#pragma unroll
    for (int c = 0; c < NCLS; ++c) p.logits[obase + c * p.oC] = l[c];
  }
  float e[NCLS], s = 0.f;
#pragma unroll
  for (int c = 0; c < NCLS; ++c) { e[c] = PRECISE ? expf(l[c] - mx) : __expf(l[c] - mx); s += e[c]; }
  const float inv = 1.0f / s;
  float pr[NCLS];
  pr[0] = PRECISE ? __fdiv_rn(e[0], s) : e[0] * inv;
  float pm = pr[0]; int am = 0;
#pragma unroll
  for (int c = 1; c < NCLS; ++c) { pr[c] = PRECISE ? __fdiv_rn(e[c], s) : e[c] * inv; if (pr[c] > pm) { pm = pr[c]; am = c; } }
  if (p.cls) p.cls[n * vox + v] = (unsigned char)am;
  if (p.probs) {
#pragma unroll
    for (int c = 0; c < NCLS; ++c) {
      float* o = p.probs + obase + c * p.oC;
      float r = p.accumulate ? __fadd_rn(*o, pr[c]) : pr[c];
      if (p.divisor != 1.0f) r = __fdiv_rn(r, p.divisor);
      *o = r;
    }
  }
}
