// What the C-ABI files (api.hip, api_infer.hip, api_aux.hip) share: the sizes a shape derives and two small helpers.
// Local to each of them (anonymous namespace): kernel files keep helpers of the same names.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/cmlpl.h"
#include "kernels.hpp"

namespace {

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

struct Dims {
  int C, H, W, bands, K, HW, H2, W2, P2, H4, W4, P4, SF, F;
};

inline bool make_dims(const cmlpl_shape* s, Dims* d) {
  if (!s) return false;
  d->C = s->C; d->H = s->H; d->W = s->W; d->bands = s->bands; d->K = s->K;
  if (d->C < 1 || d->C > 256 || d->H < 4 || d->W < 4 || d->bands < 1 || d->K < 1 || d->K > 64) return false;
  d->HW = d->H * d->W; d->H2 = d->H / 2; d->W2 = d->W / 2; d->P2 = d->H2 * d->W2;
  d->H4 = d->H2 / 2; d->W4 = d->W2 / 2; d->P4 = d->H4 * d->W4;
  d->SF = 64 * d->P4; d->F = d->SF + 1024;
  return d->P4 >= 1;
}

inline int chk(hipError_t e) { return e == hipSuccess ? 0 : (int)e; }

}  // namespace
