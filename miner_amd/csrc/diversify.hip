// diversify.hip — MMR re-ranking of ranked pools on the device (include/miner_diversify.h).
//
// One workgroup of 8 waves per user, four stages:
//   A  the pool's candidates (0 <= id < N, finite score) are compacted to the front in pool order
//      (ballot prefix; s_pos keeps the way back), so a half-empty pool costs a quarter; C of them,
//      padded to Cp = 32·ceil(C/32) with zero rows.
//   B  Gram matrix G = E·Eᵀ of the candidates' table rows on the matrix cores. The rows are gathered
//      by id in d-chunks of 128 B per row into a double-buffered LDS stage (register staging:
//      global_load_dwordx4 + ds_write_b128, one barrier per chunk; the load of chunk c+1 is in flight
//      under the products of chunk c). Stage rows are 144 B apart: the 16 rows of a ds_read_b128 lane
//      group start 36 dwords apart, 16 different 16-byte slots of the 64 banks — conflict-free.
//      Only the upper-triangular 32x32 tiles are accumulated (36 of 64 at C = 256), tile t on wave
//      t mod 8 (at most 5 accumulators, 80 registers). Both operands of a tile are rows of the stage,
//      read with ONE lane map (lane 32h + r: 16 bytes of row r at byte 32s + 16h of the chunk), so any
//      consistent split of the contraction index over steps and lane halves sums the same products:
//      fp16 / bf16 four v_mfma_f32_32x32x16 per chunk and tile, fp32 sixteen v_mfma_f32_32x32x2.
//   C  after the last chunk the stage is dead: sqrtf of the diagonal goes to s_nrm, a barrier, then
//      every tile is normalised to sim and spilled as fp32 into the packed triangle
//      tri[b(b+1)/2 + a], a <= b, which overlays the stage (C = 256: 131,584 B).
//   D  the walk: lane c < C owns compact candidate c (rel, m, taken). Each step is a wave arg-max on
//      (obj, lowest index) by shuffles, one barrier over the 4 wave results (double-buffered), and one
//      triangle read sim[c, c*] per lane to update m. Compaction keeps pool order, so the lower
//      compact index is the lower position.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "miner_diversify.h"

// the contract names every fp32 operation of the objective: no product is contracted into an fma
#pragma clang fp contract(off)

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxP = MINER_DIVERSIFY_MAX_POOL;
constexpr int kMaxD = 1024;
constexpr int kChunkB = 128;             // bytes of one row per d-chunk
constexpr int kRowStride = kChunkB + 16; // LDS bytes between stage rows
constexpr int kPieces = kMaxP * (kChunkB / 16) / kThreads;   // 16-byte pieces per thread and chunk
constexpr int kOwn = 5;                  // ceil(36 / 8) tiles per wave

struct DvParams {
  const void* news;
  const float* in_s;
  const int32_t* in_i;
  float* out_s;
  int32_t* out_i;
  int32_t* out_p;
  float* out_o;
  int N, d, P, topk, relevance;
  float lam;
};

__host__ __device__ inline int pad32(int n) { return (n + 31) & ~31; }
__host__ __device__ inline int stage_bytes(int P) { return 2 * pad32(P) * kRowStride; }
__host__ __device__ inline int tri_bytes(int P) { return pad32(P) * (pad32(P) + 1) / 2 * 4; }

__device__ __forceinline__ int acc_row(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

// acc += A·Bᵀ over the 128 bytes of one chunk; a / b point at the lane's 16 bytes of step 0
template <class T>
__device__ __forceinline__ void mma_chunk(f32x16& acc, const unsigned char* a, const unsigned char* b) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const u32x4 av = *reinterpret_cast<const u32x4*>(a + 32 * s);
    const u32x4 bv = *reinterpret_cast<const u32x4*>(b + 32 * s);
    if constexpr (__is_same(T, _Float16)) {
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, av), __builtin_bit_cast(f16x8, bv), acc, 0, 0, 0);
    } else if constexpr (__is_same(T, __bf16)) {
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, bv), acc, 0, 0, 0);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(av[i]), __uint_as_float(bv[i]), acc, 0, 0, 0);
    }
  }
}

// (obj, index) arg-max: the larger obj, then the lower index
__device__ __forceinline__ void better(float& o, int& i, float o2, int i2) {
  if (o2 > o || (o2 == o && i2 < i)) {
    o = o2;
    i = i2;
  }
}

template <class T>
__global__ __launch_bounds__(kThreads) void dv_mmr(const DvParams prm) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_big[];   // the stage, then the triangle
  __shared__ float s_score[kMaxP];
  __shared__ int s_id[kMaxP];
  __shared__ int s_pos[kMaxP];
  __shared__ float s_nrm[kMaxP];
  __shared__ float s_wmin[4], s_wmax[4];
  __shared__ int s_wcnt[4];
  __shared__ float s_robj[2][4];
  __shared__ int s_ridx[2][4];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const size_t u = blockIdx.x;
  const int P = prm.P, N = prm.N, topk = prm.topk;
  const float kInf = __builtin_huge_valf();

  // ---- A: candidates, compacted in pool order -------------------------------------------------
  float sc = 0.f;
  int id = -1;
  bool cand = false;
  if (tid < P) {
    sc = prm.in_s[u * P + tid];
    id = prm.in_i[u * P + tid];
    cand = id >= 0 && id < N && fabsf(sc) < kInf;   // false for NaN
  }
  int rank_in_wave = 0;
  if (wave < 4) {
    const unsigned long long b = __ballot(cand);
    rank_in_wave = __popcll(b & ((1ull << lane) - 1ull));
    float mn = cand ? sc : kInf, mx = cand ? sc : -kInf;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      mn = fminf(mn, __shfl_xor(mn, o, 64));
      mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    if (lane == 0) {
      s_wcnt[wave] = __popcll(b);
      s_wmin[wave] = mn;
      s_wmax[wave] = mx;
    }
  }
  __syncthreads();
  int C = 0, base = 0;
  float smin = kInf, smax = -kInf;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    if (w < wave) base += s_wcnt[w];
    C += s_wcnt[w];
    smin = fminf(smin, s_wmin[w]);
    smax = fmaxf(smax, s_wmax[w]);
  }
  C = __builtin_amdgcn_readfirstlane(C);
  if (C == 0) {                                           // nothing to list: all tails
    for (int t = tid; t < topk; t += kThreads) {
      prm.out_s[u * topk + t] = -kInf;
      prm.out_i[u * topk + t] = -1;
      prm.out_p[u * topk + t] = -1;
      if (prm.out_o) prm.out_o[u * topk + t] = -kInf;
    }
    return;
  }
  if (cand) {
    const int c = base + rank_in_wave;
    s_score[c] = sc;
    s_id[c] = id;
    s_pos[c] = tid;
  }
  __syncthreads();

  const int Cp = pad32(C);
  const int nT = Cp >> 5;
  const int ntiles = nT * (nT + 1) / 2;

  // ---- B: the Gram matrix's upper-triangular tiles ---------------------------------------------
  const int stage_half = pad32(P) * kRowStride;
  const int rowbytes = prm.d * (int)sizeof(T);
  const int nchunk = rowbytes / kChunkB;
  const int npiece = Cp * (kChunkB / 16);
  const unsigned char* tab = static_cast<const unsigned char*>(prm.news);

  const unsigned char* src[kPieces];                      // this thread's pieces: source and LDS offset
  int dst[kPieces];
#pragma unroll
  for (int k = 0; k < kPieces; ++k) {
    const int idx = tid + kThreads * k;
    const int row = idx >> 3, part = idx & 7;
    src[k] = nullptr;
    dst[k] = -1;
    if (idx < npiece) {
      dst[k] = row * kRowStride + part * 16;
      if (row < C) src[k] = tab + (size_t)s_id[row] * rowbytes + part * 16;   // padding rows stay zero
    }
  }
  int tI[kOwn], tJ[kOwn];
  f32x16 acc[kOwn];
#pragma unroll
  for (int i = 0; i < kOwn; ++i) {
    int t = wave + kWaves * i, I = 0;
    if (t < ntiles) {
      while (t >= nT - I) {
        t -= nT - I;
        ++I;
      }
    } else {
      t = 0;
    }
    tI[i] = __builtin_amdgcn_readfirstlane(I);
    tJ[i] = __builtin_amdgcn_readfirstlane(I + t);
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
  }

  u32x4 regs[kPieces];
  auto fetch = [&](int chunk) {
#pragma unroll
    for (int k = 0; k < kPieces; ++k) {
      regs[k] = u32x4{0u, 0u, 0u, 0u};
      if (src[k]) regs[k] = *reinterpret_cast<const u32x4*>(src[k] + (size_t)chunk * kChunkB);
    }
  };
  auto put = [&](int buf) {
#pragma unroll
    for (int k = 0; k < kPieces; ++k)
      if (dst[k] >= 0) *reinterpret_cast<u32x4*>(s_big + buf * stage_half + dst[k]) = regs[k];
  };
  fetch(0);
  put(0);
  __syncthreads();
  for (int c = 0; c < nchunk; ++c) {
    if (c + 1 < nchunk) fetch(c + 1);
    const unsigned char* st = s_big + (c & 1) * stage_half + r * kRowStride + h * 16;
#pragma unroll
    for (int i = 0; i < kOwn; ++i)
      if (wave + kWaves * i < ntiles)
        mma_chunk<T>(acc[i], st + tI[i] * 32 * kRowStride, st + tJ[i] * 32 * kRowStride);
    if (c + 1 < nchunk) put((c + 1) & 1);
    __syncthreads();                                      // chunk c+1 published; buffer c&1 free again
  }

  // ---- C: the diagonal's square roots, then sim into the packed triangle (over the dead stage) --
#pragma unroll
  for (int i = 0; i < kOwn; ++i)
    if (wave + kWaves * i < ntiles && tI[i] == tJ[i] && ((r >> 2) & 1) == h) {
      const int e0 = (r & 3) + 4 * (r >> 3);              // acc_row(e0, h) == r
      float g = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (e == e0) g = acc[i][e];
      s_nrm[tI[i] * 32 + r] = sqrtf(g);
    }
  __syncthreads();
  float* tri = reinterpret_cast<float*>(s_big);
#pragma unroll
  for (int i = 0; i < kOwn; ++i)
    if (wave + kWaves * i < ntiles) {
      const int b = tJ[i] * 32 + r;
      const float nb = s_nrm[b];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int a = tI[i] * 32 + acc_row(e, h);
        if (a <= b) {
          const float na = s_nrm[a];
          float sim = acc[i][e] / (na * nb);
          if (na == 0.f || nb == 0.f || !(fabsf(sim) < kInf)) sim = 0.f;
          tri[b * (b + 1) / 2 + a] = sim;
        }
      }
    }
  __syncthreads();

  // ---- D: the walk -------------------------------------------------------------------------------
  const bool mine = tid < C;
  float rel = 0.f, m = 0.f;
  if (mine) {
    const float s = s_score[tid];
    if (prm.relevance == MINER_DIVERSIFY_REL_SCORE)
      rel = s;
    else
      rel = smax == smin ? 0.f : (s - smin) / (smax - smin);
  }
  const float lam = prm.lam, oml = 1.0f - lam;
  const float lrel = lam * rel;
  bool taken = false;
  const int nsel = topk < C ? topk : C;
  for (int t = 0; t < nsel; ++t) {
    const bool open = mine && !taken;
    float obj = -kInf;
    int idx = 0x7fffffff;
    if (open) {
      obj = lrel - oml * m;
      if (obj != obj) obj = -kInf;
      idx = tid;
    }
    float bo = obj;
    int bi = idx;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float o2 = __shfl_xor(bo, o, 64);
      const int i2 = __shfl_xor(bi, o, 64);
      better(bo, bi, o2, i2);
    }
    if (wave < 4 && lane == 0) {
      s_robj[t & 1][wave] = bo;
      s_ridx[t & 1][wave] = bi;
    }
    __syncthreads();
    bo = s_robj[t & 1][0];
    bi = s_ridx[t & 1][0];
#pragma unroll
    for (int w = 1; w < 4; ++w) better(bo, bi, s_robj[t & 1][w], s_ridx[t & 1][w]);
    // an open candidate exists (t < C) and beats every closed lane's (-inf, INT_MAX): bi < C
    if (tid == bi) {
      taken = true;
      prm.out_s[u * topk + t] = s_score[tid];
      prm.out_i[u * topk + t] = s_id[tid];
      prm.out_p[u * topk + t] = s_pos[tid];
      if (prm.out_o) prm.out_o[u * topk + t] = bo;
    } else if (open) {
      const int hi = tid > bi ? tid : bi, lo = tid > bi ? bi : tid;
      const float sim = tri[hi * (hi + 1) / 2 + lo];
      m = t == 0 ? sim : fmaxf(m, sim);
    }
  }
  for (int t = nsel + tid; t < topk; t += kThreads) {
    prm.out_s[u * topk + t] = -kInf;
    prm.out_i[u * topk + t] = -1;
    prm.out_p[u * topk + t] = -1;
    if (prm.out_o) prm.out_o[u * topk + t] = -kInf;
  }
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

template <class T>
int dv_launch(void* stream, const DvParams& prm, int U) {
  auto kern = dv_mmr<T>;
  const int lds = stage_bytes(prm.P) > tri_bytes(prm.P) ? stage_bytes(prm.P) : tri_bytes(prm.P);
  hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(kern, dim3(U), dim3(kThreads), lds, static_cast<hipStream_t>(stream), prm);
  e = hipGetLastError();
  return e == hipSuccess ? MINER_OK : (int)e;
}

}  // namespace

extern "C" int miner_topk_diversify(void* stream, int dtype, const void* news, int N, int d,
                                    const float* in_scores, const int32_t* in_ids, int U, int P, int topk,
                                    float lambda, int relevance, float* out_scores, int32_t* out_ids,
                                    int32_t* out_pos, float* out_obj) {
  if (dtype != MINER_DTYPE_F32 && dtype != MINER_DTYPE_BF16 && dtype != MINER_DTYPE_F16) return MINER_EINVAL;
  if (relevance != MINER_DIVERSIFY_REL_SCORE && relevance != MINER_DIVERSIFY_REL_MINMAX) return MINER_EINVAL;
  if (U < 0 || N <= 0 || P <= 0 || topk <= 0) return MINER_EINVAL;
  if (!news || !in_scores || !in_ids || !out_scores || !out_ids || !out_pos) return MINER_EINVAL;
  if (!(lambda >= 0.f && lambda <= 1.f)) return MINER_EINVAL;
  if (P > kMaxP || topk > P) return MINER_ESHAPE;
  if (d <= 0 || d > kMaxD || d % (dtype == MINER_DTYPE_F32 ? 32 : 64)) return MINER_ESHAPE;
  if (!aligned(in_scores, 4) || !aligned(in_ids, 4) || !aligned(out_scores, 4) || !aligned(out_ids, 4) ||
      !aligned(out_pos, 4) || !aligned(out_obj, 4) || !aligned(news, 16))
    return MINER_EALIGN;
  if (U == 0) return MINER_OK;
  const DvParams prm{news, in_scores, in_ids, out_scores, out_ids, out_pos, out_obj, N, d, P, topk, relevance, lambda};
  if (dtype == MINER_DTYPE_F16) return dv_launch<_Float16>(stream, prm, U);
  if (dtype == MINER_DTYPE_BF16) return dv_launch<__bf16>(stream, prm, U);
  return dv_launch<float>(stream, prm, U);
}
