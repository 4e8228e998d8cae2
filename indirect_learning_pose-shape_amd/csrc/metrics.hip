// Segmentation metrics: the confusion matrix of (ground-truth label, arg-max prediction) counts.
//
// Reference: evaluate.py:22-127 and evaluate_autoencoder.py:23-117 (np.argmax over the 32 channels, per-class
// intersections and unions over classes 1..31, correct pixels / (W*W*num_images)) and Keras' metrics=['accuracy']
// (train.py:207-215, train_autoencoder.py:178-183, train_stage2_silhouette.py:228-234: per-pixel categorical accuracy).
// Every one of those numbers is a function of ONE matrix conf (C + 1, C): row = label (row C: a label outside [0, C)),
// column = prediction - I_k = conf[k][k], U_k = rowsum_k + colsum_k - conf[k][k], correct = trace, total = sum.
//
// A streaming kernel: 4 C bytes of scores + 4 bytes of label per pixel in, nothing per pixel out (pred_out optional).
// Lanes map onto the (npix, C) tensor as it lies in memory - VEC consecutive channels per lane (16-B loads at C = 32), a
// pixel's C channels on GL = C / VEC adjacent lanes, the arg-max across them by xor-butterfly on (score, channel) in
// torch.argmax's order (argmax_beats, common.h).  Counts go to a (C + 1) x C uint32 table in LDS (ds_add_u32 from one
// lane per pixel), and each workgroup ends with one 64-bit global atomic add per non-zero count.  Integer addition is
// associative: the result is the same bit for bit for any grid, launch order or stream.
#include "common.h"

namespace smplr {

constexpr int CONF_T = 256;       // threads per workgroup
constexpr int CONF_U = 4;         // pixels in flight per lane group (loads issued before the first is used)
constexpr int CONF_GRID = 1024;   // at most 4 workgroups per CU: the counts' flush is paid once per workgroup

template <int VEC>
struct ConfVec;
template <>
struct ConfVec<4> {
  using type = float4;
};
template <>
struct ConfVec<2> {
  using type = float2;
};
template <>
struct ConfVec<1> {
  using type = float;
};

// CT = VEC * GL channels when fixed at compile time; CT = 0: any C (VEC = GL = 1, a lane walks the pixel's channels).
template <int VEC, int GL, int CT>
__global__ __launch_bounds__(CONF_T) void seg_confusion_kernel(const float *__restrict__ scores,
                                                               const int *__restrict__ labels, long long npix, int Crt,
                                                               unsigned long long *__restrict__ conf,
                                                               unsigned char *__restrict__ pred_out) {
  static_assert(CT == 0 || CT == VEC * GL, "CT = VEC x GL");
  static_assert(CT != 0 || (VEC == 1 && GL == 1), "the any-C form takes one lane per pixel");
  const int C = CT ? CT : Crt;
  const int nconf = (C + 1) * C;
  __shared__ unsigned hist[33 * 32];
  for (int i = threadIdx.x; i < nconf; i += CONF_T) hist[i] = 0u;
  __syncthreads();
  constexpr int PPB = CONF_T / GL;                         // pixels per workgroup and step
  const int gsub = threadIdx.x % GL;
  const long long pstride = (long long)gridDim.x * PPB;
  // every lane of a pixel group takes the same trip count and the same pixel: the shuffles stay inside active groups
  for (long long p0 = (long long)blockIdx.x * PPB + threadIdx.x / GL; p0 < npix; p0 += CONF_U * pstride) {
    typename ConfVec<VEC>::type v[CONF_U];
    int lab[CONF_U];
#pragma unroll
    for (int u = 0; u < CONF_U; ++u) {
      const long long p = min(p0 + u * pstride, npix - 1);
      if (CT) {
        v[u] = *reinterpret_cast<const typename ConfVec<VEC>::type *>(scores + p * C + gsub * VEC);
      }
      lab[u] = labels[p];
    }
#pragma unroll
    for (int u = 0; u < CONF_U; ++u) {
      const long long p = p0 + u * pstride;
      float bv;
      int bi;
      if (CT) {
        const float *f = reinterpret_cast<const float *>(&v[u]);
        bv = f[0];
        bi = gsub * VEC;
#pragma unroll
        for (int t = 1; t < VEC; ++t)
          if (argmax_beats(f[t], gsub * VEC + t, bv, bi)) { bv = f[t]; bi = gsub * VEC + t; }
#pragma unroll
        for (int o = 1; o < GL; o <<= 1) {
          const float ov = __shfl_xor(bv, o, 64);
          const int oi = __shfl_xor(bi, o, 64);
          if (argmax_beats(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
      } else {
        const float *row = scores + min(p, npix - 1) * C;
        bv = row[0];
        bi = 0;
        for (int t = 1; t < C; ++t) {
          const float f = row[t];
          if (argmax_beats(f, t, bv, bi)) { bv = f; bi = t; }
        }
      }
      if (gsub == 0 && p < npix) {
        const int t = lab[u];
        atomicAdd(&hist[((unsigned)t < (unsigned)C ? t : C) * C + bi], 1u);
        if (pred_out) pred_out[p] = (unsigned char)bi;
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nconf; i += CONF_T) {
    const unsigned c = hist[i];
    if (c) atomicAdd(conf + i, (unsigned long long)c);
  }
}

// An existing prediction map (npix) int32: one lane per pixel; a prediction outside [0, C) is not counted.
__global__ __launch_bounds__(CONF_T) void seg_confusion_map_kernel(const int *__restrict__ pred,
                                                                   const int *__restrict__ labels, long long npix, int C,
                                                                   unsigned long long *__restrict__ conf,
                                                                   unsigned char *__restrict__ pred_out) {
  const int nconf = (C + 1) * C;
  __shared__ unsigned hist[33 * 32];
  for (int i = threadIdx.x; i < nconf; i += CONF_T) hist[i] = 0u;
  __syncthreads();
  const long long stride = (long long)gridDim.x * CONF_T;
  for (long long p = (long long)blockIdx.x * CONF_T + threadIdx.x; p < npix; p += stride) {
    const int k = pred[p], t = labels[p];
    if ((unsigned)k < (unsigned)C) atomicAdd(&hist[((unsigned)t < (unsigned)C ? t : C) * C + k], 1u);
    if (pred_out) pred_out[p] = (unsigned char)k;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nconf; i += CONF_T) {
    const unsigned c = hist[i];
    if (c) atomicAdd(conf + i, (unsigned long long)c);
  }
}

// workgroups for `items` lane-items of `per` per workgroup and step: at most CONF_GRID, and never so few that one
// workgroup's uint32 count could pass 2^31 pixels
static int conf_grid(long long npix, int ppb) {
  long long g = (npix + ppb - 1) / ppb;
  if (g > CONF_GRID) g = CONF_GRID;
  const long long gmin = (npix >> 31) + 1;
  return (int)(g < gmin ? gmin : g);
}

}  // namespace smplr

int smplr_seg_confusion(const float *scores, const int32_t *pred, const int32_t *labels, long long npix, int C,
                        uint64_t *conf, uint8_t *pred_out, void *stream) {
  using namespace smplr;
  SMPLR_REQUIRE(npix >= 0 && C >= 2 && C <= 32, "smplr_seg_confusion: bad sizes npix=%lld C=%d (2 <= C <= 32)", npix, C);
  SMPLR_REQUIRE((scores != nullptr) != (pred != nullptr), "smplr_seg_confusion: give exactly one of scores and pred");
  if (npix == 0) return 0;
  SMPLR_REQUIRE(labels && conf, "smplr_seg_confusion: null pointer");
  unsigned long long *cf = reinterpret_cast<unsigned long long *>(conf);
  const int *lb = reinterpret_cast<const int *>(labels);
  hipStream_t st = as_stream(stream);
  if (pred) {
    hipLaunchKernelGGL(seg_confusion_map_kernel, dim3(conf_grid(npix, CONF_T)), dim3(CONF_T), 0, st,
                       reinterpret_cast<const int *>(pred), lb, npix, C, cf, pred_out);
    SMPLR_LAUNCH_CHECK("smplr_seg_confusion");
    return 0;
  }
  const uintptr_t al = reinterpret_cast<uintptr_t>(scores);
#define SMPLR_CONF_LAUNCH(VEC_, GL_, CT_)                                                                            \
  hipLaunchKernelGGL((seg_confusion_kernel<VEC_, GL_, CT_>), dim3(conf_grid(npix, CONF_T / GL_)), dim3(CONF_T), 0, st, \
                     scores, lb, npix, C, cf, pred_out)
  // (the vector forms need the base aligned to their load; a tensor view that is not falls to the any-C form)
  if (C == 32 && al % 16 == 0) SMPLR_CONF_LAUNCH(4, 8, 32);
  else if (C == 16 && al % 16 == 0) SMPLR_CONF_LAUNCH(4, 4, 16);
  else if (C == 8 && al % 16 == 0) SMPLR_CONF_LAUNCH(4, 2, 8);
  else if (C == 4 && al % 16 == 0) SMPLR_CONF_LAUNCH(4, 1, 4);
  else if (C == 2 && al % 8 == 0) SMPLR_CONF_LAUNCH(2, 1, 2);
  else SMPLR_CONF_LAUNCH(1, 1, 0);
#undef SMPLR_CONF_LAUNCH
  SMPLR_LAUNCH_CHECK("smplr_seg_confusion");
  return 0;
}
