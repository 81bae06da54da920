// corpus.hip — full-corpus ranking for MI355X (gfx950 / CDNA4): BASELINE config 5, SURVEY.md §7
// step 6 ("a users x news GEMM with fused softmax-over-K and a top-k epilogue; output never
// materialised"). Two kernels:
//
//   ue_fused  user encoder, one workgroup (8 waves) per user, any L <= 256 and K <= 64:
//             PolyAttention (model.py:159-185) -> mui [K,d] and proj = gelu(mui·W2ᵀ) (model.py:212)
//     S1+S2  wave w owns history rows [32w, 32w+32): Pᵀ = tanh(W1·Eᵀ) for all 8 Dc-tiles (Dc padded
//            to 256 with zero weights) and then Sᵀ = Q·Pᵀ straight from the accumulators — no
//            cross-wave exchange; Sᵀ (+ bias) -> LDS
//     S3     masked softmax over L per interest (masked logits = 1e-30, model.py:180)
//     S4     muiᵀ = Eᵀ·Aᵀ over 32-row slabs of E LDS-DMA'd twice-buffered (16-bit: ds_read_b64_tr_b16
//            Eᵀ fragments), wave w owning d-tiles w, w+8, ...
//     S5     per interest tile: the mui image in LDS, projᵀ = gelu(W2·muiᵀ), W2 streamed (packed)
//
//   rk_fused  ranker: workgroup tile = 2 users x 256 news per step, contraction over d in 128-byte
//             chunks staged through LDS by LDS-DMA (double buffered, XOR-swizzled rows); wave w owns
//             user w>>2 and news [64(w&3), +64) and holds all of that user's K-row tiles (proj and
//             mui) for its 64 news, so the click score (softmax over K of proj·e weighting mui·e,
//             model.py:127-134, 213-214) is an in-register epilogue plus one lane-half exchange. Each
//             workgroup owns whole users: a running top-k per user in LDS, threshold-filtered, so
//             the U x N scores never leave the CU. Two more forms of the same kernel share its
//             contraction and score epilogue bit for bit: the counting form (per user and target,
//             how many news rank before it: exact full-corpus ranks without a list) and the pair
//             form (the scores of a per-user id list, U x C rows only).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <stdint.h>
#include <math.h>
#include <utility>

#include "../../include/miner_corpus.h"
#include "cdna4_common.h"

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = 8;
constexpr int kMaxL = MINER_CORPUS_MAX_L;
constexpr int kMaxK = MINER_CORPUS_MAX_K;
constexpr int kMaxTopk = MINER_CORPUS_MAX_TOPK;
constexpr int kDcT = 8;          // Dc padded to 8 tiles of 32
constexpr int kMaxD = 768;

inline bool aligned16(const void* q) { return q == nullptr || (reinterpret_cast<uintptr_t>(q) & 15u) == 0; }
inline bool aligned4(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 3u) == 0; }

int num_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    cus = n;
  }
  return cus;
}

__device__ __forceinline__ int fresh_lane() {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return t & 63;
}

template <class T> __device__ __forceinline__ float cx_exp(float x) {
  if constexpr (sizeof(T) == 2) return __expf(x); else return expf(x);
}
template <class T> __device__ __forceinline__ float cx_tanh(float x) {
  if constexpr (sizeof(T) == 2) return tanh_fast(x); else return tanhf(x);
}
__device__ __forceinline__ float xor32_max(float x) {
  const auto s = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(s[0]), __uint_as_float(s[1]));
}
__device__ __forceinline__ float xor32_sum(float x) {
  const auto s = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(s[0]) + __uint_as_float(s[1]);
}
__device__ __forceinline__ float wave_max(float x) {
  x = row16_max(x);
  const auto s = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return xor32_max(fmaxf(__uint_as_float(s[0]), __uint_as_float(s[1])));
}
__device__ __forceinline__ float wave_sum(float x) {
  x = row16_sum(x);
  const auto s = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return xor32_sum(__uint_as_float(s[0]) + __uint_as_float(s[1]));
}

// ================================================================================================
// user encoder
// ================================================================================================
// packed weights (T elements): W1p [8 ct][ns] blocks (rows 32ct + pi(rr) of W1, zero past Dc),
// Qp [nkt][8 c] blocks (rows 32kt + pi(rr) of Q, columns 32c.., zero past K / Dc),
// W2p [ns][ns] blocks (rows 32jt + pi(rr) of W2); each block fragment-major (cdna4_common.h)
__host__ __device__ inline size_t ue_w1_elems(int d) { return (size_t)kDcT * (d >> 5) * 1024; }
__host__ __device__ inline size_t ue_q_elems(int K) { return (size_t)((K + 31) >> 5) * kDcT * 1024; }
__host__ __device__ inline size_t ue_w2_elems(int d) { return (size_t)(d >> 5) * (d >> 5) * 1024; }

template <class T>
__global__ void ue_pack_kernel(const T* __restrict__ W1, const T* __restrict__ Q, const T* __restrict__ W2, int d,
                               int Dc, int K, T* __restrict__ out) {
  const size_t n1 = ue_w1_elems(d), nq = ue_q_elems(K), n2 = W2 ? ue_w2_elems(d) : 0;
  const int ns = d >> 5;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n1 + nq + n2; i += (size_t)gridDim.x * blockDim.x) {
    T v = (T)0.f;
    int rr, cc;
    block_pos<T>((int)(i & 1023), rr, cc);
    if (i < n1) {
      const int tile = (int)(i >> 10), ct = tile / ns, j = tile % ns;
      const int row = 32 * ct + pi_row(rr);
      if (row < Dc) v = W1[(size_t)row * d + 32 * j + cc];
    } else if (i < n1 + nq) {
      const int tile = (int)((i - n1) >> 10), kt = tile / kDcT, c = tile % kDcT;
      const int row = 32 * kt + pi_row(rr), col = 32 * c + cc;
      if (row < K && col < Dc) v = Q[(size_t)row * Dc + col];
    } else {
      const int tile = (int)((i - n1 - nq) >> 10), jt = tile / ns, j = tile % ns;
      v = W2[(size_t)(32 * jt + pi_row(rr)) * d + 32 * j + cc];
    }
    out[i] = v;
  }
}

struct UeParams {
  const void* hist;        // dense [U, L, d], or the news table (gather)
  const int32_t* his_ids;  // [U, L] or null
  int n_news;
  const uint8_t* mask;
  const float* bias;
  const void* wp;
  float* mui_f32;          // [U, K, d] or null
  void* user_mui;          // [U, K, d] T
  void* user_proj;         // [U, K, d] T or null
  int U, L, d, Dc, K;
};

// LDS carve (bytes)
constexpr int kSS = kMaxL + 4;                          // S / fp32-A row stride (floats)
constexpr int kSBytes = kMaxK * kSS * 4;                // logits; fp32 mode: A in place
// mui image row stride (elements): an odd number of 16-byte units, so the 16 rows of a ds_read_b128
// lane group land in 16 different bank slots
template <class T> constexpr int kMS = kMaxD + 16 / (int)sizeof(T);
template <class T> constexpr int kMuiImg = 32 * kMS<T> * (int)sizeof(T);  // one interest tile
template <class T> constexpr int kEBuf = sizeof(T) == 2 ? 32 * kMaxD * 2 : 0;  // one E slab image (16-bit)
template <class T> constexpr int kR1 = ((kSBytes > kMuiImg<T> ? kSBytes : kMuiImg<T>) > 2 * kEBuf<T>
                                            ? (kSBytes > kMuiImg<T> ? kSBytes : kMuiImg<T>) : 2 * kEBuf<T>);
constexpr int kAS = kMaxL + 8;                          // 16-bit A row stride (elements)
template <class T> constexpr int kABytes = sizeof(T) == 2 ? kMaxK * kAS * 2 : 0;
template <class T> constexpr int kOffA = kR1<T>;
template <class T> constexpr int kOffIds = kOffA<T> + kABytes<T>;
template <class T> constexpr int kOffZero = kOffIds<T> + kMaxL * 4;
template <class T> constexpr int kUeLds = kOffZero<T> + 64;
static_assert(kUeLds<__bf16> <= 160 * 1024 && kUeLds<float> <= 160 * 1024, "encoder LDS");

// A-operand fragment of Eᵀ (rows = columns i0 + pi(..) of E, contraction over the 32 rows of an
// E slab image) via ds_read_b64_tr_b16; rows >= nvalid read the zero block
template <class T>
__device__ __forceinline__ void frag_load_Et(Frag<T>& bf, unsigned img_off, unsigned zero_off, int i0, int rowB,
                                             int g16, int nvalid, int lane) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
  const int col = i0 + 16 * (pp & 1) + 8 * (g & 1) + 4 * (pp >> 1);
  const int ch = col >> 3, sub8 = (col & 7) * 2;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int row = 16 * (g >> 1) + 8 * s + 4 * u + q;
      const unsigned off = row < nvalid ? img_off + row * rowB + ((ch ^ eswz(row, g16)) << 4) + sub8 : zero_off;
      const i16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4*)((lds_char*)smem + off));
      bf.q[s][2 * u] = (unsigned)(unsigned short)v[0] | ((unsigned)(unsigned short)v[1] << 16);
      bf.q[s][2 * u + 1] = (unsigned)(unsigned short)v[2] | ((unsigned)(unsigned short)v[3] << 16);
    }
  }
}

// nrows rows of d elements (dense from src, or table rows ids[r]) -> an E slab image (whole 1 KiB
// DMA blocks; chunk c of row `row` at c ^ eswz(row))
template <class T>
__device__ __forceinline__ void ue_dma_slab(const T* src, const int32_t* idsL, int n_news, int nrows, int d,
                                            char* img, int wave, int lane) {
  const int cpr = d >> 3;
  const int g16 = (cpr & 15) == 0;
  const int total = nrows * cpr;
  const int nblk = (total + 63) >> 6;
  for (int blk = wave; blk < nblk; blk += kWaves) {
    const int pos = blk * 64 + lane;
    const int row = pos / cpr;
    const int c = pos - row * cpr;
    const int rr = min(row, nrows - 1);
    const size_t r = idsL ? (size_t)min(max(idsL[rr], 0), n_news - 1) : (size_t)rr;
    const T* g = (pos < total) ? src + r * d + (size_t)((c ^ eswz(row, g16)) << 3) : src;
    dma_b128(g, __builtin_amdgcn_readfirstlane(lds_offset(img + blk * 1024)));
  }
}

template <class T, int NKT, bool GATHER>
__global__ __launch_bounds__(kThreads) void ue_fused(UeParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr bool k16 = sizeof(T) == 2;
  const int L = p.L, d = p.d, K = p.K, ns = d >> 5;
  const int nLt = (L + 31) >> 5;
  const T* __restrict__ W1p = static_cast<const T*>(p.wp);
  const T* __restrict__ Qp = W1p + ue_w1_elems(d);
  const T* __restrict__ W2p = Qp + ue_q_elems(K);
  float* S = reinterpret_cast<float*>(smem);
  int32_t* idsL = reinterpret_cast<int32_t*>(smem + kOffIds<T>);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (threadIdx.x < 16) reinterpret_cast<float*>(smem + kOffZero<T>)[threadIdx.x] = 0.f;

  for (int u = blockIdx.x; u < p.U; u += gridDim.x) {
    const T* __restrict__ base = static_cast<const T*>(p.hist) + (GATHER ? (size_t)0 : (size_t)u * L * d);
    if constexpr (GATHER) {
      __syncthreads();      // the previous user's readers of the id block are done
      for (int i = threadIdx.x; i < L; i += kThreads) idsL[i] = p.his_ids[(size_t)u * L + i];
    }
    __syncthreads();

    // ---- S1 + S2: wave w = history rows [32w, 32w + 32) ----
    if (wave < nLt) {
      const int lane = fresh_lane();
      const int r = lane & 31, h = lane >> 5;
      const int m = min(32 * wave + r, L - 1);
      const T* erow = GATHER ? base + (size_t)min(max(idsL[m], 0), p.n_news - 1) * d : base + (size_t)m * d;
      f32x16 acc[kDcT];
#pragma unroll
      for (int c = 0; c < kDcT; ++c) acc[c] = zero16();
      for (int j = 0; j < ns; ++j) {
        Frag<T> eb;
        frag_load<T>(eb, erow + 32 * j + 16 * h);
#pragma unroll
        for (int c = 0; c < kDcT; ++c) {
          Frag<T> wa;
          frag_load_tile<T>(wa, W1p + (size_t)(c * ns + j) * 1024, lane);
          mma_slab<T>(acc[c], wa, eb);          // Pᵀ[dc][l] over this d slab
        }
      }
      f32x16 sacc[NKT];
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) sacc[kt] = zero16();
#pragma unroll
      for (int c = 0; c < kDcT; ++c) {
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[c][e] = cx_tanh<T>(acc[c][e]);     // model.py:171
        Frag<T> pf;
        acc_to_frag<T>(pf, acc[c]);            // lane (h, l): 16 consecutive Dc of row l
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
          Frag<T> qa;
          frag_load_tile<T>(qa, Qp + (size_t)(kt * kDcT + c) * 1024, lane);
          mma_slab<T>(sacc[kt], qa, pf);        // Sᵀ[k][l] (model.py:174)
        }
      }
      const int l = 32 * wave + r;
      const float bl = (p.bias && l < L) ? p.bias[(size_t)u * L + l] : 0.f;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
#pragma unroll
        for (int e = 0; e < 16; ++e) S[(32 * kt + 16 * h + e) * kSS + l] = sacc[kt][e] + bl;   // + bias (model.py:176)
      }
    }
    __syncthreads();

    // ---- S3: masked softmax over the history (model.py:178-181), 8 interests per wave ----
    {
      const int lane = fresh_lane();
      const uint8_t* mrow = p.mask + (size_t)u * L;
      bool real[kMaxL / 64];
#pragma unroll
      for (int i = 0; i < kMaxL / 64; ++i) {
        const int l = lane + 64 * i;
        real[i] = l < L && mrow[min(l, L - 1)] != 0;
      }
#pragma unroll
      for (int q = 0; q < 32 * NKT / kWaves; ++q) {
        const int k = wave * (32 * NKT / kWaves) + q;
        float v[kMaxL / 64];
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < kMaxL / 64; ++i) {
          const int l = lane + 64 * i;
          v[i] = l < L ? (real[i] ? S[k * kSS + l] : 1e-30f) : -INFINITY;
          mx = fmaxf(mx, v[i]);
        }
        mx = wave_max(mx);
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < kMaxL / 64; ++i) {
          v[i] = (lane + 64 * i < L) ? cx_exp<T>(v[i] - mx) : 0.f;
          sum += v[i];
        }
        sum = wave_sum(sum);
        const float inv = k < K ? 1.0f / sum : 0.f;
#pragma unroll
        for (int i = 0; i < kMaxL / 64; ++i) {
          const int l = lane + 64 * i;
          if constexpr (k16) reinterpret_cast<T*>(smem + kOffA<T>)[k * kAS + l] = (T)(v[i] * inv);
          else S[k * kSS + l] = v[i] * inv;    // in place: this lane read exactly these entries
        }
      }
    }
    __syncthreads();

    // ---- S4: muiᵀ = Eᵀ · Aᵀ, wave w owning d-tiles w, w + 8, ... ----
    constexpr int kDt = kMaxD / 32 / kWaves;    // d-tiles per wave (<= 3)
    f32x16 macc[kDt][NKT];
#pragma unroll
    for (int i = 0; i < kDt; ++i)
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) macc[i][kt] = zero16();
    if constexpr (k16) {
      const int rowB = 2 * d, g16 = (((d >> 3) & 15) == 0);
      const int nls = nLt;
      {
        const int lane = fresh_lane();
        ue_dma_slab<T>(base, GATHER ? idsL : nullptr, p.n_news, min(32, L), d, smem, wave, lane);
      }
      for (int s = 0; s < nls; ++s) {
        vm_wait_all();
        __syncthreads();      // slab s landed; slab s - 1's buffer is free
        const int lane = fresh_lane();
        const int r = lane & 31, h = lane >> 5;
        if (s + 1 < nls) {
          const int r0 = 32 * (s + 1);
          ue_dma_slab<T>(GATHER ? base : base + (size_t)r0 * d, GATHER ? idsL + r0 : nullptr, p.n_news,
                         min(32, L - r0), d, smem + ((s + 1) & 1) * kEBuf<T>, wave, lane);
        }
        const unsigned img = lds_offset(smem + (s & 1) * kEBuf<T>);
        const unsigned zoff = lds_offset(smem + kOffZero<T>);
        const int nvalid = min(32, L - 32 * s);
        Frag<T> af[NKT];
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
          frag_load<T>(af[kt], reinterpret_cast<const T*>(smem + kOffA<T>) + (32 * kt + r) * kAS + 32 * s + 16 * h);
#pragma unroll
        for (int i = 0; i < kDt; ++i) {
          const int dt = wave + kWaves * i;
          if (dt < ns) {
            Frag<T> ef;
            frag_load_Et<T>(ef, img, zoff, 32 * dt, rowB, g16, nvalid, lane);
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt) mma_slab<T>(macc[i][kt], ef, af[kt]);   // lane (h,k): d 16h..
          }
        }
      }
    } else {
      // fp32 parity mode: E columns straight from L2 (one element per register), A rows natural
      const int lane = fresh_lane();
      const int r = lane & 31, h = lane >> 5;
      for (int s = 0; s < nLt; ++s) {
        Frag<T> af[NKT];
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) frag_load<T>(af[kt], S + (32 * kt + r) * kSS + 32 * s + 16 * h);
#pragma unroll
        for (int i = 0; i < kDt; ++i) {
          const int dt = wave + kWaves * i;
          if (dt < ns) {
            Frag<T> ef;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
              const int l = min(32 * s + 16 * h + e, L - 1);      // rows >= L: finite x zero weight
              const size_t row = GATHER ? (size_t)min(max(idsL[l], 0), p.n_news - 1) : (size_t)l;
              ef.q[e >> 2][e & 3] = __float_as_uint(base[row * d + 32 * dt + r]);
            }
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt) mma_slab<T>(macc[i][kt], af[kt], ef);   // lane (h,d): k rows
          }
        }
      }
    }
    __syncthreads();          // E slab buffers / A free: the mui images go there

    // ---- outputs: mui, then S5 per interest tile ----
    {
      const int lane = fresh_lane();
      const int r = lane & 31, h = lane >> 5;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        T* img = reinterpret_cast<T*>(smem);         // [32 k][kMS]
#pragma unroll
        for (int i = 0; i < kDt; ++i) {
          const int dt = wave + kWaves * i;
          if (dt >= ns) continue;
          if constexpr (k16) {
            const int k = 32 * kt + r;
            Frag<T> mf;
            acc_to_frag<T>(mf, macc[i][kt]);
            frag_store<T>(img + r * kMS<T> + 32 * dt + 16 * h, mf);
            if (k < K) {
              frag_store<T>(static_cast<T*>(p.user_mui) + ((size_t)u * K + k) * d + 32 * dt + 16 * h, mf);
              if (p.mui_f32) {
                float4* o = reinterpret_cast<float4*>(p.mui_f32 + ((size_t)u * K + k) * d + 32 * dt + 16 * h);
#pragma unroll
                for (int g = 0; g < 4; ++g)
                  o[g] = float4{macc[i][kt][4 * g], macc[i][kt][4 * g + 1], macc[i][kt][4 * g + 2], macc[i][kt][4 * g + 3]};
              }
            }
          } else {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
              const int kl = acc_row(e, h), k = 32 * kt + kl;
              img[kl * kMS<T> + 32 * dt + r] = macc[i][kt][e];
              if (k < K) {
                static_cast<T*>(p.user_mui)[((size_t)u * K + k) * d + 32 * dt + r] = macc[i][kt][e];
                if (p.mui_f32) p.mui_f32[((size_t)u * K + k) * d + 32 * dt + r] = macc[i][kt][e];
              }
            }
          }
        }
        if (p.user_proj) {
          __syncthreads();    // the mui image of this interest tile is complete
          // projᵀ = gelu(W2 · muiᵀ): wave w owns W2 row tiles w, w + 8, ...
#pragma unroll
          for (int i = 0; i < kDt; ++i) {
            const int jt = wave + kWaves * i;
            if (jt >= ns) continue;
            f32x16 pacc = zero16();
            for (int j = 0; j < ns; ++j) {
              Frag<T> wa, mb;
              frag_load_tile<T>(wa, W2p + (size_t)(jt * ns + j) * 1024, lane);
              frag_load<T>(mb, img + r * kMS<T> + 32 * j + 16 * h);
              mma_slab<T>(pacc, wa, mb);
            }
            gelu_tile<T>(pacc);                         // model.py:212 (exact erf in fp32 mode)
            const int k = 32 * kt + r;
            if (k < K) {
              Frag<T> pf;
              acc_to_frag<T>(pf, pacc);
              frag_store<T>(static_cast<T*>(p.user_proj) + ((size_t)u * K + k) * d + 32 * jt + 16 * h, pf);
            }
          }
        }
        __syncthreads();      // before the next interest tile's image (or the next user) reuses LDS
      }
    }
  }
}

// ================================================================================================
// ranker
// ================================================================================================
constexpr int kUT = 2;            // users per workgroup tile
constexpr int kNT = 256;          // news per step

struct RkParams {
  const void* mui;
  const void* proj;
  const void* news;
  float* top_s;
  int32_t* top_i;
  float* ws_s;             // S > 1: per (user, news slice) top-k lists [U][S][topk], merged by rk_merge
  int32_t* ws_i;
  size_t ws_bytes;         // the caller's workspace size (the split form needs U·S·topk·8)
  const int32_t* excl;     // [U][E] news ids a user's list must not hold (NULL / E = 0: none)
  const uint32_t* ok;      // ceil(N / 32) words, bit n & 31 of word n >> 5: news n may be ranked (NULL: all)
  int U, N, d, K, topk, score_type, E;
  const int32_t* ids;      // SUB: the news rows to rank, news[ids[pos]] for pos in [0, M); distinct ids
  int M;                   //      (pair form: [U][M], user u's list at ids + u·M; repeats allowed)
  const float* tgt_s;      // counting form: [U][T] target scores and ids; the counts go to top_i [U][T]
  const int32_t* tgt_i;
  int T;
  const float* bias;       // BIAS: the score priors [G][N] fp32, added to every score before it is used
  const int32_t* grp;      //       [U] prior rows (NULL: row 0 for every user), clamped into [0, G)
  int G;
  const int32_t* clus;     // CAP: the cluster table [N] (< 0: in no cluster); a list holds at most cap news
  int cap;                 //      of one cluster
  const float* aft_s;      // AFT: the keyset cursors [U] (NULL: none); user u's list holds only what ranks
  const int32_t* aft_i;    //      strictly after (aft_s[u], aft_i[u])
  int32_t* top_g;          // INT: the dominant interests out — pair form [U][M] next to the scores; capped form
  int icap;                //      [U][topk] next to the list (NULL: not wanted). icap > 0: the per-interest cap
                           //      as the caller gave it; the kernel reads it as `cap` (rk_run), as the capped form does
  const int32_t* use_g;    // CAP | AFT, the resumed walk: per user the groups already served, [U][Q] strictly ascending,
  const int32_t* use_c;    //      their counts [U][Q] (< 0 reads as 0) and the number of pairs [U] (clamped into
  const int32_t* use_n;    //      [0, Q] on the device); a group's in-list rank starts at its count instead of 0
  int Q;
};

// S > 1 (S = 8, grid = 256): the news steps are dealt to S slices (step st of slice s is news step
// s + S·st) and 8 consecutive user tiles x 8 slices go to the 32 workgroups b that share b % 8 — one
// XCD under the round-robin placement (speed only, never correctness): workgroup b takes slice
// (b >> 3) & 7 of the tiles 32 r + 4 (b & 7) + ((b >> 6) & 3), r = 0, 1, ... So an XCD's L2 holds the
// user rows of 8 users (1.5 MB at K = 64, d = 768, both mui and proj) that its 32 CUs all read,
// and every news row it fetches serves 8 users; with S = 1 every CU streams its own 2 users' rows
// (12 MB per XCD, beyond its 4 MB L2) and the table once per 2 users.
constexpr int kSplit = 8;

// diagnostic builds only (tools/rk_ablate.py): bit 1 no DMAs, 2 no MFMAs, 4 no epilogue, 8 no
// per-chunk barrier (the results are wrong, only the time is read)
#ifndef MINER_RK_ABL
#define MINER_RK_ABL 0
#endif
#ifndef MINER_RK_DMAW
#define MINER_RK_DMAW 4   // 91.5 -> 86.9 ms per config-5 step against 8 (tools/rk_ablate.py)
#endif

// one LDS-DMA (saddr form: scalar base + 32-bit per-lane offset) into M0 = m, M0 saved / restored;
// default cache policy (nt on the ranker's rows cost 18 %, tools/rk_ablate.py)
__device__ __forceinline__ void rk_dma(uint32_t off, const char* base, unsigned m) {
  unsigned t;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(t) : "v"(off), "s"(base), "s"(m) : "memory");
}

// image geometry: rows of RB bytes per chunk; 16-byte unit c of row `row` at c ^ rk_swz(row) —
// RB = 128: (row >> 1) & 7, RB = 64: (row >> 2) & 3. Either way the 16 rows of a ds_read_b128 lane
// group (natural or pi order: lanes {0-3, 12-15, 20-27} read rows {0-3, 12-15, 20-27}) land in 16
// different 16-byte bank slots.
template <int RB>
__device__ __forceinline__ int rk_swz(int row) { return RB == 128 ? (row >> 1) & 7 : (row >> 2) & 3; }

template <class T, int RB>
__device__ __forceinline__ void rk_frag(Frag<T>& f, const char* img, int row, int c0) {
#pragma unroll
  for (int i = 0; i < kNQ<T>; ++i)
    f.q[i] = *reinterpret_cast<const u32x4*>(img + row * RB + (((c0 + i) ^ rk_swz<RB>(row)) << 4));
}

// a wave's vector-memory operations down to N outstanding
template <int N>
__device__ __forceinline__ void vm_wait_n() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }

// stream geometry: GEO 0 rows of 128 B, a ring of 2 stages (the next chunk in flight); GEO 1 (16-bit,
// at least two row tiles per user) rows of 64 B, a ring of 4 stages of the same total size (three
// chunks in flight)
template <int GEO> constexpr int kRB = GEO ? 64 : 128;
template <int GEO> constexpr int kRing = GEO ? 4 : 2;

// a wave-uniform word from global memory through the scalar cache (s_load, counted by lgkmcnt, not
// behind the vector loads and LDS-DMAs in flight)
__device__ __forceinline__ unsigned rk_sload(const uint32_t* q) {
  return *(const __attribute__((address_space(4))) uint32_t*)(uintptr_t)q;
}

// total order of ranked entries: higher score first, then lower news id
__device__ __forceinline__ bool better(float s, int i, float s2, int i2) { return s > s2 || (s == s2 && i < i2); }

// The same order as one unsigned 64-bit compare, for the counting form: better(s, i, s2, i2) ==
// (key(s, i) > key(s2, i2)) with key = rk_okey(score) << 32 | rk_ikey(id), for scores that are not
// NaN. rk_okey: the float's bits made monotone (-0 taken as +0, as the float compare takes it;
// integer operations only, so nothing is rounded or flushed); every real score, -inf included, has
// a key half >= 0x007fffff. rk_ikey: a lower (signed) id gives a greater key.
__device__ __forceinline__ unsigned rk_okey(float s) {
  unsigned u = __float_as_uint(s);
  if (u == 0x80000000u) u = 0u;
  return u ^ ((unsigned)((int)u >> 31) | 0x80000000u);
}
__device__ __forceinline__ unsigned rk_ikey(int id) { return (unsigned)id ^ 0x7fffffffu; }

template <int NR, int GEO = 0, bool FLT = false, bool CAP = false, bool INT = false>
struct RkLds {
  static constexpr int kARows = kUT * NR * 32;
  static constexpr int kStage = (kARows + kNT) * kRB<GEO>;
  static constexpr int kOffList = kRing<GEO> * kStage;              // [kUT][kMaxTopk] float + int
  static constexpr int kOffStage = kOffList + kUT * kMaxTopk * 8;  // staged candidates [2 bufs][kUT][kNT]
  static constexpr int kOffCnt = kOffStage + 2 * kUT * kNT * 8;     // list counts [kUT], staged [2][kUT]
  static constexpr int kOffExcl = kOffCnt + 64;                     // the tile's exclusion lists [kUT][kMaxL] int
  // CAP: per list entry its cluster id and its rank inside its cluster, [kUT][kMaxTopk] int each,
  // then the cluster ids of the staged entries being merged [kUT][kNT] (INT: the interests staged with
  // the entries by the epilogue, double buffered as the staging area is, [2 bufs][kUT][kNT])
  static constexpr int kOffClus = kOffExcl + (FLT ? kUT * kMaxL * 4 : 0);
  static constexpr int kTotal = kOffClus + (CAP ? (2 * kUT * kMaxTopk + (INT ? 2 : 1) * kUT * kNT) * 4 : 0);
};

// NCH: RB-byte d-chunks per row (0: at run time); GEO: the stream geometry (kRB / kRing); FLT: the
// filtered form (RkParams excl / ok). A compile-time switch: as run-time branches on the two pointers
// the unfiltered config-5 step measured 79.5 against the parent's 76.0 ms (profiles/rk_filter_ab.txt).
// SUB: the subset form (RkParams ids / M; always with FLT, either filter may be null). The news
// steps, slices and tiles run over the positions pos in [0, M) of the id list; the row of position
// pos is news[ids[pos]], gathered with one address per lane; a candidate's identity — in the
// threshold test, the filters and the staged entry — is its table id ids[pos], so the list does not
// depend on the order of the ids.
// MODE: what the epilogue does with a score. kRank: the running top-k above. kCount (the counting
// form, RkParams tgt_s / tgt_i / T): no list; every score of an eligible news (the bitmap, rows < N)
// is compared with the tile's targets, [kUT][kMaxT] (score, id) pairs in LDS (as 64-bit keys in the
// ranker's order, rk_okey / rk_ikey), and per target the scores that rank before it are counted —
// lane j of a wave keeps its count for target j, the user's
// four nsub waves are summed in LDS at the tile's end and counts[u][0..T) leaves in one vector store
// (S = 1: a user belongs to one workgroup, so no atomics and a deterministic result). kPair (the
// pair form, with SUB): a tile is ONE user, in both uu slots, against 256 entries per step of that
// user's own id list ids[u][0..M); the score goes to top_s[u][pos], -inf for an id outside [0, N).
// The d-chunk loop, the K reductions and the lane-half exchanges are the ones of kRank, so a pair's
// score has the same bits in all three.
// BIAS: the biased forms (RkParams bias / grp / G; the ranking forms always with FLT, as SUB). The
// score of (user u, news n) becomes fp32_add_rn(score, bias[group(u)][n]) — one separate IEEE add
// (rk_add_rn) on the finished score — before the threshold test, the key compare or the store, so
// lists, counts and pair scores agree bit for bit with "scores + prior" in fp32. A compile-time
// switch for the reason FLT is one: the unbiased instantiations are the same code as without it.
// AFT: the cursor form (RkParams aft_s / aft_i; kRank, GEO 0, filtered — either filter may be null —,
// split or unsplit; with CAP only as the resumed walk, below). A compile-time switch on the biased instantiation with the prior
// tested at run time (the CAP pattern): as a run-time test on p.aft_s in the filtered instantiations
// the filtered config-5 step without a cursor measured 81.27 against the parent's 80.39 ms, outside
// the parent's own 0.74 ms spread (the two cursor words live in scalar registers across the step
// loop), so every instantiation a call without a cursor launches is the code it was. A candidate
// (score, n) of user u is kept only if better(aft_s[u], aft_i[u], score, n) — the ranked value (the biased sum under a prior) and the table id (ids[pos] in the subset form),
// compared exactly as the threshold test compares, from the other side. So a cursor of +inf / -1 is
// before every listable entry, -inf / 2^31 - 1 after all of them, a NaN cursor score lists nothing,
// and a cursor that is no listable news is a position in the order like any other. The running
// list, the staging, the merge and rk_merge never see an entry at or before the cursor: each slice
// of the split form applies it, and split and unsplit agree bit for bit.
// CAP: the capped form (RkParams clus / cap; kRank, unsplit, GEO 0, filtered). A user's list is the
// greedy walk of its ranking that keeps an entry iff fewer than cap better entries of its cluster
// were kept — a mergeable summary as the top-k is, so only the merge changes (below): the contraction,
// the epilogue, the threshold test and the staging are the uncapped form's, and a listed score has
// its bits. To keep the build small the CAP instantiations are the BIAS ones with the prior tested at
// run time (no table: nothing is loaded and nothing is added, so an unbiased capped score is not
// "score + 0"); CAP is a compile-time switch so that every other instantiation is the code it was.
// INT: the interest forms (RkParams top_g / icap). interest(u, n) is the lowest k in [0, K) whose value
// equals the maximum the score's own K reduction found — over the logits proj_k · e_n ('weighted': the
// mx of the softmax) or over M_k ('max': the score itself) —, -1 if none compares equal (all NaN). It
// is read off the accumulators the score was made from, after the contraction (rk_interest), so no
// score bit changes, and a prior never enters it. Accumulator e of lane half h in interest tile kt
// is interest 32 kt + 16 h + e (the row of the user image that lane pi_row⁻¹ loaded: pi_row(acc_row(e,
// h)) = 16 h + e), the index the K mask of the epilogue uses. kPair | INT: the interest is stored
// next to the score, top_g[u][pos] (-1 for an id outside [0, N)). CAP | INT: the capped form with the
// group of an entry its interest instead of clus[id]: computed lazily, only by the half-waves that
// stage something (bal != 0; the accumulators are still live there), staged with the entry (stg_g,
// double buffered) and read by the capped merge in place of its table loads; the list's groups leave
// with the list (top_g, when wanted). Never for the mean score, which has no dominant interest (the
// INT forms are not instantiated for it).
// CAP | AFT (with or without INT): the resumed capped walk (RkParams use_g / use_c / use_n / Q next to
// the cursor). The walk of the capped form continued strictly after the cursor, with used(g) entries
// of group g already served: an entry is kept iff its group is negative or used(g) + (the better kept
// entries of g in this call) < cap. "Keep the best cap - used(g) of group g" is a mergeable summary as
// the capped list is, so the epilogue is the cursor form's (the AFT test on the ranked value and the
// table id) and the capped merge changes in one place: a staged entry's in-group rank starts at
// used(its group) instead of 0 (list entries carry theirs). used() is a lower-bound search of the
// user's strictly ascending group table in global memory (L2-resident, at most 8 KB per user; at
// K = 64, d = 768 with CAP | INT 8 KB of LDS remain, which two users x 1,024 pairs do not fit), made
// by the merging wave where it loads the staged entries' cluster ids — nothing else of that wave is
// in flight there —, at most 11 dependent loads per merge whatever the number of staged entries, and
// skipped wholesale for an empty table. The table pointer and its length are per (tile, user), set in
// the tile loop next to the cursor words: a workgroup's later tiles never read an earlier tile's.
// Compile-time forms of their own: every instantiation a call without a state launches is the code
// it was.
constexpr int kRank = 0, kCount = 1, kPair = 2;
constexpr int kMaxT = MINER_CORPUS_MAX_TARGETS;

// a + b rounded once to nearest even, never contracted with the operation that made a (the divide
// of the mean and weighted scores): the compiler cannot see through the barrier
__device__ __forceinline__ float rk_add_rn(float a, float b) {
  asm volatile("" : "+v"(a));
  return __fadd_rn(a, b);
}

// A form: every compile-time switch of rk_fused but T / NKT / SCORE, in one word — the switches
// above as named bits, kCount / kPair for MODE (neither: kRank), kFSplit for S = kSplit, and the
// shape bits of the launcher (kFD768: NCH = 768 · 2 / RB, kFK64: KC = 64; 0 is "at run time").
constexpr unsigned kFFlt = 1, kFSub = 2, kFBias = 4, kFCap = 8, kFAft = 16, kFGeo1 = 32, kFSplit = 64, kFCount = 128,
                   kFPair = 256, kFD768 = 512, kFK64 = 1024, kFInt = 2048;
template <unsigned F>
struct RkForm {
  static constexpr bool FLT = F & kFFlt, SUB = F & kFSub, BIAS = F & kFBias, CAP = F & kFCap, AFT = F & kFAft;
  static constexpr bool INT = F & kFInt;
  static constexpr int MODE = F & kFCount ? kCount : F & kFPair ? kPair : kRank;
  static constexpr int S = F & kFSplit ? kSplit : 1, GEO = F & kFGeo1 ? 1 : 0;
  static constexpr int NCH = F & kFD768 ? 768 * 2 / kRB<GEO> : 0, KC = F & kFK64 ? 64 : 0;   // KC: K compile-time (0: run time)
  static_assert(F < 2 * kFInt && (F & (kFCount | kFPair)) != (kFCount | kFPair) && (!(F & kFK64) || (F & kFD768)), "a form");
  static_assert(!AFT || (MODE == kRank && GEO == 0 && FLT && BIAS), "the cursor form: filtered, on the biased form (with CAP: the resumed walk)");
  static_assert(!CAP || (MODE == kRank && S == 1 && GEO == 0 && FLT && BIAS), "the capped form: unsplit, filtered, on the biased form");
  static_assert(!INT || MODE == kPair || CAP, "the interest forms: the pair form and the capped form");
  static_assert(!SUB || (FLT && GEO == 0), "the subset form: a filtered form with one chunk in flight");
  static_assert(!BIAS || (GEO == 0 && (FLT || MODE == kCount)), "the biased forms: GEO 0, the ranking forms filtered");
  static_assert(MODE == kRank || (S == 1 && GEO == 0 && SUB == (MODE == kPair)), "counting and pair forms: unsplit, GEO 0");
};

// INT: the dominant interest of this lane's news from the NKT accumulator tiles lg[0 .. NKT) the K
// reduction ran over and the maximum mx it found (the same in both lane halves): per lane the lowest
// k of its half's elements that compare equal to mx (walked downwards, so the last hit is the
// lowest), then the lane-half exchange the maximum made, taking the lower; -1 if no element compares
// equal. All 64 lanes take part.
constexpr int kNoInterest = 0x7fffffff;
template <int NKT>
__device__ __forceinline__ int rk_interest(const f32x16 (*lg)[2], int nt, float mx, int h, int K) {
  int kk = kNoInterest;
#pragma unroll
  for (int kt = NKT - 1; kt >= 0; --kt)
#pragma unroll
    for (int e = 15; e >= 0; --e) {
      const int k = 32 * kt + 16 * h + e;
      if (k < K && lg[kt][nt][e] == mx) kk = k;
    }
  const auto s = __builtin_amdgcn_permlane32_swap((unsigned)kk, (unsigned)kk, false, false);
  kk = min((int)s[0], (int)s[1]);
  return kk == kNoInterest ? -1 : kk;
}

template <class T, int NKT, int SCORE, unsigned F>
__global__ __launch_bounds__(kThreads) void rk_fused(RkParams p) {
  using Fm = RkForm<F>;
  constexpr int NCH = Fm::NCH, S = Fm::S, GEO = Fm::GEO, KC = Fm::KC, MODE = Fm::MODE;
  constexpr bool FLT = Fm::FLT, SUB = Fm::SUB, BIAS = Fm::BIAS, CAP = Fm::CAP, AFT = Fm::AFT, INT = Fm::INT;
  static_assert(!INT || SCORE != MINER_SCORE_MEAN, "the mean score has no dominant interest");
  static_assert((NCH == 0 || sizeof(T) == 2) && (KC == 0 || NKT == 2), "the compile-time shape: 16-bit, K = 64 on two interest tiles");
  constexpr bool kRtPrior = CAP || AFT;             // BIAS instantiations that test the prior at run time
  static_assert(kMaxT == 64 && kUT * kMaxT * 8 <= kUT * kMaxTopk * 8 && kUT * 4 * kMaxT * 4 <= 2 * kUT * kNT * 8,
                "one target per lane; the targets in the list area, the partial counts in the staging area");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr bool kW = SCORE == MINER_SCORE_WEIGHTED;
  constexpr int NR = kW ? 2 * NKT : NKT;            // row tiles per user: mui (and proj)
  constexpr int RB = kRB<GEO>, RING = kRing<GEO>, PD = RING - 1;   // PD: chunks in flight
  using LD = RkLds<NR, GEO, FLT, CAP, INT>;
  constexpr int kChunkSlabs = RB / (32 * (int)sizeof(T));          // 32-index slabs per chunk
  static_assert(kChunkSlabs >= 1, "a chunk holds whole slabs");
  const int d = NCH > 0 ? NCH * RB / (int)sizeof(T) : p.d, K = KC > 0 ? KC : p.K, N = p.N;
  const int nchunk = NCH > 0 ? NCH : d * (int)sizeof(T) / RB;
  const int NP = SUB ? p.M : N;                                    // news positions: table rows, or list entries
  const int nsteps = ((NP + kNT - 1) / kNT + S - 1) / S;           // news steps per slice
  const int ntiles = MODE == kPair ? p.U : (p.U + kUT - 1) / kUT;   // pair form: a tile is one user
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int uu = wave >> 2, nsub = wave & 3;
  float* list_s = reinterpret_cast<float*>(smem + LD::kOffList);
  int* list_i = reinterpret_cast<int*>(smem + LD::kOffList + kUT * kMaxTopk * 4);
  float* stg_s = reinterpret_cast<float*>(smem + LD::kOffStage);                    // [buf][uu][kNT]
  int* stg_i = reinterpret_cast<int*>(smem + LD::kOffStage + 2 * kUT * kNT * 4);
  int* cnt = reinterpret_cast<int*>(smem + LD::kOffCnt);   // [0, kUT) list sizes, kUT + buf * kUT + uu staged
  int* excl = reinterpret_cast<int*>(smem + LD::kOffExcl);  // [kUT][kMaxL], -1 past E (FLT and p.E > 0 only)
  [[maybe_unused]] int* list_g = reinterpret_cast<int*>(smem + LD::kOffClus);                   // CAP: [kUT][kMaxTopk]
  [[maybe_unused]] int* list_r = reinterpret_cast<int*>(smem + LD::kOffClus + kUT * kMaxTopk * 4);
  [[maybe_unused]] int* stg_g = reinterpret_cast<int*>(smem + LD::kOffClus + 2 * kUT * kMaxTopk * 4);   // [kUT][kNT]; INT: [buf][kUT][kNT]
  // counting form (no list, nothing staged): the targets [kUT][kMaxT] and the waves' partial counts [kWaves][kMaxT]
  [[maybe_unused]] unsigned* tg_h = reinterpret_cast<unsigned*>(smem + LD::kOffList);   // key halves: score, id
  [[maybe_unused]] unsigned* tg_l = reinterpret_cast<unsigned*>(smem + LD::kOffList + kUT * kMaxT * 4);
  [[maybe_unused]] int* part = reinterpret_cast<int*>(smem + LD::kOffStage);
  static_assert(kUT * kMaxL == kThreads && kMaxL == 4 * 64, "one exclusion slot per thread, four per lane of a wave");
  // the user's merging wave: 0 and 5 (two SIMDs under the wave -> SIMD w % 4 placement)
  const bool merger = wave == 5 * uu;
  const T* __restrict__ mui = static_cast<const T*>(p.mui);
  const T* __restrict__ proj = static_cast<const T*>(p.proj);
  const T* __restrict__ news = static_cast<const T*>(p.news);
  const int b = blockIdx.x;
  const int first = S == 1 ? b : 4 * (b & 7) + ((b >> 6) & 3);    // this workgroup's first tile
  const int tstride = S == 1 ? (int)gridDim.x : 32;
  const int slice = S == 1 ? 0 : (b >> 3) & 7;
  if (first >= ntiles) return;
  const int ntile_mine = (ntiles - first + tstride - 1) / tstride;
  const int total_chunks = ntile_mine * nsteps * nchunk;
  auto news_step = [&](int st) { return S == 1 ? st : slice + S * st; };

  // Row DMAs. Wave w issues the 1 KiB blocks w + 8 j of every stage: j < NR are user k-rows (A),
  // the rest news rows (B). The per-lane byte offsets are fixed for the launch (A: within the user's
  // [K, d] array; B: from the step's first news row); the user, step and chunk go into the scalar
  // base of the saddr form. A chunk's blocks are issued spread over the previous chunk's MFMAs.
  constexpr int kBlk = (LD::kARows + kNT) * RB / 1024;              // 1 KiB DMA blocks per stage
  static_assert(kBlk % kWaves == 0, "whole DMA blocks per wave");
  constexpr int kJ = kBlk / kWaves;
  constexpr int kUnits = RB / 16;                                    // 16-byte units per row
  constexpr int kRpb = 1024 / RB;                                    // rows per DMA block
  constexpr int kAJ = LD::kARows / (kWaves * kRpb);                  // A blocks per wave (jj < kAJ)
  static_assert(LD::kARows % (kWaves * kRpb) == 0, "A blocks split evenly over the waves");
  uint32_t voff[kJ];
#pragma unroll
  for (int jj = 0; jj < kJ; ++jj) {
    const int lane = fresh_lane();
    const int P = (wave + kWaves * jj) * 64 + lane;
    const int row = P / kUnits, cl = (P % kUnits) ^ rk_swz<RB>(row);
    if (jj < kAJ) {
      const int k = min(32 * (((row >> 5) % NR) % NKT) + (row & 31), K - 1);
      voff[jj] = (uint32_t)(k * d) * (uint32_t)sizeof(T) + cl * 16;
    } else if constexpr (SUB) {
      voff[jj] = cl * 16;                                            // the row comes from the id list
    } else {
      voff[jj] = (uint32_t)((row - LD::kARows) * d) * (uint32_t)sizeof(T) + cl * 16;
    }
  }
  // the next chunk to issue: (tile nti, slice step nsl, chunk nc), advanced after each issue
  int nti = first, nsl = 0, nc = 0;
  // SUB: the table rows of this lane's news blocks in the issue pointer's step nsl (not the step
  // being computed: the issue side runs PD chunks ahead, across step and tile boundaries), loaded
  // when nsl moves. Positions at or past M take the list's last entry, and an id is clamped into
  // [0, N) before it becomes an address (neither is ever a candidate, see the epilogue).
  int bid[SUB ? kJ : 1];
  auto load_bids = [&]() {
    if constexpr (SUB) {
      const int lane = fresh_lane();
      const int st = S == 1 ? nsl : slice + S * nsl;
      // pair form: the list of the user being ISSUED (tile nti; past the last tile — nothing more
      // is issued then — the last user's, so the read stays inside the array)
      const int32_t* ids = MODE == kPair ? p.ids + (size_t)min(nti, p.U - 1) * p.M : p.ids;
#pragma unroll
      for (int jj = kAJ; jj < kJ; ++jj) {
        const int row = ((wave + kWaves * jj) * 64 + lane) / kUnits;
        const int pos = min(st * kNT + (row - LD::kARows), p.M - 1);
        bid[jj] = min(max(ids[pos], 0), N - 1);
      }
    }
  };
  // the id registers' loads complete here, behind a wait the caller has just made (the compiler's
  // own wait before their first use would otherwise land behind freshly issued DMAs)
  auto pin_bids = [&]() {
    if constexpr (SUB) {
#pragma unroll
      for (int jj = kAJ; jj < kJ; ++jj) asm volatile("" : "+v"(bid[jj]));
    }
  };
  load_bids();
  auto dma_block = [&](int jj, int stage) {
    const unsigned la = __builtin_amdgcn_readfirstlane(lds_offset(smem + stage * LD::kStage + (wave + kWaves * jj) * 1024));
    if (jj < kAJ) {
      const int row0 = (wave + kWaves * jj) * kRpb;
      const int t = (row0 >> 5) % NR, ou = row0 / (NR * 32);
      const int user = min(MODE == kPair ? nti : nti * kUT + ou, p.U - 1);
      const T* src = (kW && t >= NKT) ? proj : mui;
      rk_dma(voff[jj], reinterpret_cast<const char*>(src + (size_t)user * K * d) + nc * RB, la);
    } else if constexpr (SUB) {
      // one 64-bit address per lane: the table row of this lane's position, chunk nc, unit voff
      const char* row = reinterpret_cast<const char*>(news) + (size_t)bid[jj] * ((size_t)d * sizeof(T));
      dma_b128_rt(row + nc * RB + voff[jj], la);
    } else {
      const int st = news_step(nsl);
      if (st * kNT + kNT <= N) {
        rk_dma(voff[jj], reinterpret_cast<const char*>(news + (size_t)st * kNT * d) + nc * RB, la);
      } else {                           // the table's last (partial) step: rows clamped to N - 1
        const int lane = fresh_lane();
        const int P = (wave + kWaves * jj) * 64 + lane;
        const int row = P / kUnits, cl = (P % kUnits) ^ rk_swz<RB>(row);
        const int n = min(st * kNT + (row - LD::kARows), N - 1);
        dma_b128_rt(news + (size_t)n * d + nc * (RB / (int)sizeof(T)) + cl * (16 / (int)sizeof(T)), la);
      }
    }
  };
  auto advance = [&]() {
    if (++nc == nchunk) {
      nc = 0;
      if (++nsl == nsteps) { nsl = 0; nti += tstride; }
      load_bids();
    }
  };

  if (wave >= 4) __builtin_amdgcn_s_setprio(1);   // static priority for the second half (-0.8 %)
  if (threadIdx.x < 3 * kUT) cnt[threadIdx.x] = 0;

  // CAP | AFT: the served-group table of this wave's user in the tile being computed (set in the tile
  // loop, read by the merges of that tile only)
  [[maybe_unused]] int use_n = 0;
  [[maybe_unused]] const int32_t* use_g = nullptr;
  [[maybe_unused]] const int32_t* use_c = nullptr;

  // merge the candidates staged in buffer `buf` into user uu's running top-k (one wave). The list
  // (best first) and the staged entries are ranked in parallel: an entry's new position is the
  // number of entries of both sets better than it (a total order on distinct news ids); entries
  // ranked past topk drop out. Every LDS read comes before the first write (one wave, in order).
  auto merge = [&](int buf) {
    const int ns = cnt[kUT + buf * kUT + uu];
    if (ns == 0) return;
    const int lane = fresh_lane();
    const int c = cnt[uu];
    float* ls = list_s + uu * kMaxTopk;
    int* li = list_i + uu * kMaxTopk;
    const float* ss = stg_s + (buf * kUT + uu) * kNT;
    const int* si = stg_i + (buf * kUT + uu) * kNT;
    constexpr int kLT = kMaxTopk / 64, kST = kNT / 64;
    float lv[kLT], sv[kST];
    int lid[kLT], sid[kST], lr[kLT], sr[kST];
    if constexpr (CAP) {
      // The capped merge: the capped list of (list ∪ staged). The list is a valid capped list, so
      // each entry carries its cluster id and its rank inside its cluster (list_g / list_r).
      // Pass 1: per entry of both sets, rc = the better entries of its own cluster in the union (a
      // list entry: its carried rank plus the better staged ones); kept iff unclustered or rc < cap
      // — the better entries of a kept entry's cluster are then kept too, so rc is also its rank
      // among the kept and is carried on. Pass 2: an entry's position = the better KEPT entries (the
      // list's: a prefix count of its kept mask). Every read of the list and of the staging buffer
      // comes before the first write to the list.
      // The staged entries' cluster ids are loaded HERE, by the one merging wave, first of all: the
      // merge runs at a step's first chunk between the chunk's wait and the next chunk's DMA issue,
      // so nothing else of this wave is in flight and the wait below is for these loads alone (the
      // tile's last merge waits for the next tile's first chunk once). A load in the epilogue, by
      // the staging lanes, would be waited with vmcnt(0) behind the next chunk's row DMAs on every
      // wave that staged something.
      int* lg_ = list_g + uu * kMaxTopk;
      int* lrk_ = list_r + uu * kMaxTopk;
      // INT: the groups are the interests the epilogue staged with the entries: nothing is loaded
      // from global memory and the staged array itself is what the walk below reads.
      int* mg = stg_g + (INT ? buf * kUT + uu : uu) * kNT;
      int sg[kST], lg[kLT], lrc[kLT], src[kST];
#pragma unroll
      for (int v = 0; v < kST; ++v) {
        const int j = min(lane + 64 * v, kNT - 1);
        sv[v] = ss[j];
        sid[v] = si[j];
        if constexpr (INT) sg[v] = lane + 64 * v < ns ? mg[j] : -1;
        else sg[v] = lane + 64 * v < ns ? p.clus[sid[v]] : -1;   // a staged id is a table row: inside [0, N)
        src[v] = 0;
      }
      if constexpr (AFT) {
        // the resumed walk: src starts at used(sg) — the lower bound of sg in the user's ascending
        // group table, the same number of steps for every lane (the range halves each time, so
        // floor(log2 use_n) + 1 steps empty it), every address clamped into [0, use_n)
        if (use_n > 0) {
          int lo[kST], hi[kST];
#pragma unroll
          for (int v = 0; v < kST; ++v) { lo[v] = 0; hi[v] = use_n; }
          for (int it = 0; (use_n >> it) > 0; ++it) {
#pragma unroll
            for (int v = 0; v < kST; ++v) {
              const int mid = min((lo[v] + hi[v]) >> 1, use_n - 1);
              const int gm = use_g[mid];
              if (lo[v] < hi[v]) {
                if (gm < sg[v]) lo[v] = mid + 1; else hi[v] = mid;
              }
            }
          }
#pragma unroll
          for (int v = 0; v < kST; ++v) {
            const int at = min(lo[v], use_n - 1);
            const int gm = use_g[at], cm = use_c[at];
            if (sg[v] >= 0 && lo[v] < use_n && gm == sg[v]) src[v] = max(cm, 0);
          }
        }
      }
#pragma unroll
      for (int t = 0; t < kLT; ++t) {
        const int i = min(lane + 64 * t, kMaxTopk - 1);
        const bool in = lane + 64 * t < c;
        lv[t] = ls[i];
        lid[t] = li[i];
        lg[t] = in ? lg_[i] : -1;
        lrc[t] = lrk_[i];
      }
      if constexpr (!INT) {
#pragma unroll
        for (int v = 0; v < kST; ++v) mg[lane + 64 * v] = sg[v];
      }
      for (int j2 = 0; j2 < ns; ++j2) {
        const int g2 = __builtin_amdgcn_readfirstlane(mg[j2]);
        if (g2 < 0) continue;                    // never capped, and in nobody's cluster
        const float s2 = ss[j2];
        const int i2 = si[j2];
        int nl = 0;                              // better list entries of cluster g2
#pragma unroll
        for (int t = 0; t < kLT; ++t) {
          const bool same = lg[t] == g2;
          lrc[t] += same && better(s2, i2, lv[t], lid[t]) ? 1 : 0;
          nl += __popcll(__ballot(same && better(lv[t], lid[t], s2, i2)));
        }
#pragma unroll
        for (int v = 0; v < kST; ++v) {
          src[v] += sg[v] == g2 && better(s2, i2, sv[v], sid[v]) ? 1 : 0;
          if (j2 == lane + 64 * v) src[v] += nl;
        }
      }
      bool lk[kLT], sk[kST];
      unsigned long long lkm[kLT], skm[kST];
      int kept = 0;
#pragma unroll
      for (int t = 0; t < kLT; ++t) {
        lk[t] = lane + 64 * t < c && (lg[t] < 0 || lrc[t] < p.cap);
        lkm[t] = __ballot(lk[t]);
        lr[t] = kept + __popcll(lkm[t] & ((1ull << lane) - 1));   // the better kept list entries
        kept += __popcll(lkm[t]);
      }
#pragma unroll
      for (int v = 0; v < kST; ++v) {
        sk[v] = lane + 64 * v < ns && (sg[v] < 0 || src[v] < p.cap);
        skm[v] = __ballot(sk[v]);
        kept += __popcll(skm[v]);
        sr[v] = 0;
      }
      for (int j2 = 0; j2 < ns; ++j2) {
        const unsigned long long m = j2 < 64 ? skm[0] : j2 < 128 ? skm[1] : j2 < 192 ? skm[2] : skm[3];
        static_assert(kST == 4, "four staged masks");
        if (!((m >> (j2 & 63)) & 1)) continue;   // wave-uniform: a dropped entry displaces nothing
        const float s2 = ss[j2];
        const int i2 = si[j2];
        int nl = 0;
#pragma unroll
        for (int t = 0; t < kLT; ++t) {
          lr[t] += better(s2, i2, lv[t], lid[t]) ? 1 : 0;
          nl += __popcll(__ballot(lk[t] && better(lv[t], lid[t], s2, i2)));
        }
#pragma unroll
        for (int v = 0; v < kST; ++v) {
          sr[v] += better(s2, i2, sv[v], sid[v]) ? 1 : 0;
          if (j2 == lane + 64 * v) sr[v] += nl;
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int t = 0; t < kLT; ++t) {
        if (lk[t] && lr[t] < p.topk) {
          ls[lr[t]] = lv[t];
          li[lr[t]] = lid[t];
          lg_[lr[t]] = lg[t];
          lrk_[lr[t]] = lrc[t];
        }
      }
#pragma unroll
      for (int v = 0; v < kST; ++v) {
        if (sk[v] && sr[v] < p.topk) {
          ls[sr[v]] = sv[v];
          li[sr[v]] = sid[v];
          lg_[sr[v]] = sg[v];
          lrk_[sr[v]] = src[v];
        }
      }
      if (lane == 0) {
        cnt[uu] = min(kept, p.topk);
        cnt[kUT + buf * kUT + uu] = 0;
      }
      return;
    }
#pragma unroll
    for (int t = 0; t < kLT; ++t) {
      const int i = min(lane + 64 * t, kMaxTopk - 1);
      lv[t] = ls[i];
      lid[t] = li[i];
      lr[t] = lane + 64 * t;
    }
#pragma unroll
    for (int v = 0; v < kST; ++v) {
      const int j = min(lane + 64 * v, kNT - 1);
      sv[v] = ss[j];
      sid[v] = si[j];
      sr[v] = 0;
    }
    for (int j2 = 0; j2 < ns; ++j2) {
      const float s2 = ss[j2];
      const int i2 = si[j2];
      int nl = 0;                              // list entries better than staged entry j2
#pragma unroll
      for (int t = 0; t < kLT; ++t) {
        lr[t] += better(s2, i2, lv[t], lid[t]) ? 1 : 0;   // staged entries better than each entry
        nl += __popcll(__ballot(lane + 64 * t < c && better(lv[t], lid[t], s2, i2)));
      }
#pragma unroll
      for (int v = 0; v < kST; ++v) {
        sr[v] += better(s2, i2, sv[v], sid[v]) ? 1 : 0;
        if (j2 == lane + 64 * v) sr[v] += nl;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int t = 0; t < kLT; ++t) {
      if (lane + 64 * t < c && lr[t] < p.topk) {
        ls[lr[t]] = lv[t];
        li[lr[t]] = lid[t];
      }
    }
#pragma unroll
    for (int v = 0; v < kST; ++v) {
      if (lane + 64 * v < ns && sr[v] < p.topk) {
        ls[sr[v]] = sv[v];
        li[sr[v]] = sid[v];
      }
    }
    if (lane == 0) {
      cnt[uu] = min(c + ns, p.topk);
      cnt[kUT + buf * kUT + uu] = 0;
    }
  };

  for (int q0 = 0; q0 < PD && q0 < total_chunks; ++q0) {   // prologue: the first PD chunks
    if (!(MINER_RK_ABL & 1)) {
#pragma unroll
      for (int jj = 0; jj < kJ; ++jj) dma_block(jj, q0);
    }
    advance();
  }
  int q = 0;
  int nid[2] = {-1, -1};       // SUB: the table ids of this lane's news columns in the step being computed
  // BIAS: the priors of those two news for user uu (0 where there is no news): pri in the step being
  // computed, pnx in the step after it (the next tile's first step after a tile's last), loaded a
  // step ahead — at a step's first chunk, when nothing of this wave is in flight — so that every path
  // from the load to the epilogue that adds it passes a chunk's wait: issued in the epilogue, or
  // used in the step that loads it, the load is waited with vmcnt(0) behind the row DMAs of the
  // chunk in flight. The gathering forms load the next step's ids (idn) the same way and the priors
  // at those ids one chunk later (a one-chunk step: at once, behind a wait of their own).
  [[maybe_unused]] float pri[2] = {0.f, 0.f}, pnx[2] = {0.f, 0.f};
  [[maybe_unused]] int idn[2] = {-1, -1};
  [[maybe_unused]] const float* prow = nullptr;   // the prior row of pnx's user
  // the prior row of the user in this wave's uu slot of tile t (the two users of a tile may read
  // different rows); a user past U takes the last user's and a group outside [0, G) is clamped, so
  // no address leaves the table
  auto prior_row = [&](int t) -> const float* {
    if constexpr (kRtPrior) if (p.bias == nullptr) return nullptr;   // (the capped / cursor form without a prior)
    const int bu = min(MODE == kPair ? t : t * kUT + uu, p.U - 1);
    int g = 0;
    if (p.grp != nullptr) g = (int)rk_sload(reinterpret_cast<const uint32_t*>(p.grp) + bu);
    return p.bias + (size_t)min(max(g, 0), p.G - 1) * (size_t)N;
  };
  auto load_idn = [&](int t, int s) {             // SUB: as nid, for slice step s of tile t
    const int lane = fresh_lane();
    const int32_t* ids = MODE == kPair ? p.ids + (size_t)t * p.M : p.ids;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int pos = news_step(s) * kNT + 64 * nsub + 32 * nt + (lane & 31);
      const int id = ids[min(pos, p.M - 1)];
      idn[nt] = pos < p.M && (unsigned)id < (unsigned)N ? id : -1;
    }
  };
  auto load_pnx = [&](int s) {                    // one coalesced 128-byte load per (nt, user)
    const int lane = fresh_lane();
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int n = SUB ? idn[nt] : news_step(s) * kNT + 64 * nsub + 32 * nt + (lane & 31);
      pnx[nt] = (!kRtPrior || p.bias != nullptr) && (SUB ? n >= 0 : n < N) ? prow[n] : 0.f;
    }
  };
  if constexpr (BIAS) {                           // the first step's (complete behind the first chunk's wait)
    prow = prior_row(first);
    if constexpr (SUB) load_idn(first, 0);
    load_pnx(0);
  }
  for (int ti = first; ti < ntiles; ti += tstride) {
    // the tile's exclusion lists (the previous tile's epilogues are behind its closing barriers; this
    // tile's first epilogue comes after a chunk barrier). A user past U and slots past E hold -1.
    if (FLT && p.E > 0) {
      const int eu = ti * kUT + (int)(threadIdx.x / kMaxL), es = threadIdx.x % kMaxL;
      excl[threadIdx.x] = eu < p.U && es < p.E ? p.excl[(size_t)eu * p.E + es] : -1;
    }
    // counting form: the tile's targets as keys (rk_okey / rk_ikey), at the same point and under the
    // same barriers. A slot past T, or of a user past U, and a target whose score is NaN hold the
    // greatest key: nothing ranks before it.
    int tcount = 0;            // this wave's count for target `lane` of user uu, over the tile's steps
    if constexpr (MODE == kCount) {
      if (threadIdx.x < kUT * kMaxT) {
        const int eu = ti * kUT + (int)(threadIdx.x / kMaxT), es = threadIdx.x % kMaxT;
        const bool in = eu < p.U && es < p.T;
        const float s = in ? p.tgt_s[(size_t)eu * p.T + es] : NAN;
        const int id = in ? p.tgt_i[(size_t)eu * p.T + es] : 0;
        tg_h[threadIdx.x] = s == s ? rk_okey(s) : 0xffffffffu;
        tg_l[threadIdx.x] = s == s ? rk_ikey(id) : 0xffffffffu;
      }
    }
    // the cursor of this wave's user: two wave-uniform words through the scalar cache, once per
    // (tile, user), held in scalar registers across the step loop (complete long before the first
    // epilogue; never a vector load behind the row DMAs). A user past U reads the last user's and
    // is never a candidate.
    [[maybe_unused]] float aft_s = INFINITY;
    [[maybe_unused]] int aft_i = -1;
    if constexpr (AFT) {
      const int au = min(ti * kUT + uu, p.U - 1);
      aft_s = __uint_as_float(rk_sload(reinterpret_cast<const uint32_t*>(p.aft_s) + au));
      aft_i = (int)rk_sload(reinterpret_cast<const uint32_t*>(p.aft_i) + au);
      if constexpr (CAP) {
        // the resumed walk: this tile's user's group table, its length a wave-uniform word clamped
        // into [0, Q] so that no address leaves the table (a user past U: the last user's, never read
        // — it stages nothing)
        use_n = min(max((int)rk_sload(reinterpret_cast<const uint32_t*>(p.use_n) + au), 0), p.Q);
        use_g = p.use_g + (size_t)au * p.Q;
        use_c = p.use_c + (size_t)au * p.Q;
      }
    }
    for (int sl = 0; sl < nsteps; ++sl) {
      const int st = news_step(sl);
      f32x16 acc[NR][2];
#pragma unroll
      for (int t = 0; t < NR; ++t) { acc[t][0] = zero16(); acc[t][1] = zero16(); }
      for (int c = 0; c < nchunk; ++c, ++q) {
        // chunk q landed (this wave's DMAs of chunks q + 1 .. q + PD - 1 may stay in flight), then
        // for every wave; chunk q - 1's stage is free
        if (!(MINER_RK_ABL & 1)) {
          if (PD > 1 && q + PD - 1 < total_chunks) vm_wait_n<(PD - 1) * kJ>();
          else vm_wait_all();
        }
        if (!(MINER_RK_ABL & 8)) __syncthreads();
        if constexpr (SUB) {
          // nothing of this wave is in flight: the id loads of advance() and of the step's first chunk
          // are complete without a wait of their own. Then, at a step's first chunk, the table ids of
          // this lane's two news columns, once per step (-1: no candidate).
          pin_bids();
          asm volatile("" : "+v"(nid[0]), "+v"(nid[1]));
          if (c == 0) {
            const int lane = fresh_lane();
            // (pair form: the list of the user being COMPUTED, tile ti)
            const int32_t* ids = MODE == kPair ? p.ids + (size_t)ti * p.M : p.ids;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
              const int pos = st * kNT + 64 * nsub + 32 * nt + (lane & 31);
              const int id = ids[min(pos, p.M - 1)];
              nid[nt] = pos < p.M && (unsigned)id < (unsigned)N ? id : -1;
            }
          }
        }
        if constexpr (BIAS) {
          // what was loaded for the next step is complete behind the wait above (pinned, as the ids
          // are); at a step's first chunk it becomes this step's, and the step after is loaded
          asm volatile("" : "+v"(pnx[0]), "+v"(pnx[1]));
          if constexpr (SUB) asm volatile("" : "+v"(idn[0]), "+v"(idn[1]));
          if (c == 0) { pri[0] = pnx[0]; pri[1] = pnx[1]; }
          const bool wrap = sl + 1 == nsteps;
          const int t2 = wrap ? ti + tstride : ti, s2 = wrap ? 0 : sl + 1;
          if (t2 < ntiles) {
            if (c == 0) {
              if (wrap) prow = prior_row(t2);
              if constexpr (SUB) load_idn(t2, s2);
            }
            if (c == (SUB && nchunk > 1 ? 1 : 0)) load_pnx(s2);
          }
        }
        // the previous step's staged candidates (its epilogue is behind this barrier); the next
        // epilogue reads the list only after this chunk's barriers
        if (MODE == kRank && c == 0 && sl > 0 && merger && !(MINER_RK_ABL & 4)) merge((sl - 1) & 1);
        const bool pre = !(MINER_RK_ABL & 1) && q + PD < total_chunks;
        const int lane = fresh_lane();
        const int r = lane & 31, h = lane >> 5;
        const char* img = smem + (q % RING) * LD::kStage;
        const char* bimg = img + LD::kARows * RB;
        constexpr int kPairs = kChunkSlabs * NR;
#pragma unroll
        for (int s = 0; s < kChunkSlabs; ++s) {
          const int c0 = (2 * s + h) * kNQ<T>;
          Frag<T> bf[2];
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) rk_frag<T, RB>(bf[nt], bimg, 64 * nsub + 32 * nt + r, c0);
#pragma unroll
          for (int t = 0; t < NR; ++t) {
            Frag<T> af;
            rk_frag<T, RB>(af, img, (uu * NR + t) * 32 + pi_row(r), c0);
            if (!(MINER_RK_ABL & 2)) {
              mma_slab<T>(acc[t][0], af, bf[0]);
              mma_slab<T>(acc[t][1], af, bf[1]);
            } else {
              acc[t][0][0] += __builtin_bit_cast(float, af.q[0][0]);   // keep the reads
              acc[t][1][0] += __builtin_bit_cast(float, bf[1].q[0][0]);
            }
            // the next chunk's DMA blocks, spread over this chunk's first kWin MFMA pairs
            constexpr int kWin = MINER_RK_DMAW < kPairs ? MINER_RK_DMAW : kPairs;
#pragma unroll
            for (int jj = 0; jj < kJ; ++jj)
              if (jj * kWin / kJ == s * NR + t && pre) dma_block(jj, (q + PD) % RING);
          }
        }
        if (pre) advance();
      }
      if (nchunk == 1 && sl > 0) __syncthreads();   // (one chunk per step: the merge above is done)
      // ---- epilogue: click score of (user uu, news) for this wave's 64 news ----
      if (MINER_RK_ABL & 4) {            // every accumulator stays live (no MFMA is dead code)
        float z = 0.f;
#pragma unroll
        for (int t = 0; t < NR; ++t)
#pragma unroll
          for (int e = 0; e < 16; ++e) z += acc[t][0][e] + acc[t][1][e];
        if (z == 1234.5f) p.top_s[0] = z;
      } else {
        const int lane = fresh_lane();
        const int r = lane & 31, h = lane >> 5;
        const int user = ti * kUT + uu;
        const float th_s = (MODE != kRank || cnt[uu] < p.topk) ? -INFINITY : list_s[uu * kMaxTopk + p.topk - 1];
        const int th_i = (MODE != kRank || cnt[uu] < p.topk) ? 0x7fffffff : list_i[uu * kMaxTopk + p.topk - 1];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          // the candidate's identity: its table row (SUB: of this position's id, -1 for "none")
          const int n = SUB ? nid[nt] : st * kNT + 64 * nsub + 32 * nt + r;
          float score;
          [[maybe_unused]] float kmx = 0.f;          // INT: the maximum of the K reduction
          if constexpr (kW) {
            // 4 independent max / sum chains per lane (a 32-long dependent chain each otherwise)
            float m4[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
              for (int e = 0; e < 16; ++e)
                if (32 * kt + 16 * h + e < K) m4[e & 3] = fmaxf(m4[e & 3], acc[NKT + kt][nt][e]);
            const float mx = xor32_max(fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3])));
            kmx = mx;
            float s0[4] = {0.f, 0.f, 0.f, 0.f}, s1[4] = {0.f, 0.f, 0.f, 0.f};
            // 16-bit: exp(x - mx) as exp2(x·log2 e - mx·log2 e), one fma + v_exp_f32 per interest
            const float mxl = mx * 1.44269504088896340736f;
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
              for (int e = 0; e < 16; ++e)
                if (32 * kt + 16 * h + e < K) {
                  const float lg = acc[NKT + kt][nt][e];
                  const float ex = sizeof(T) == 2 ? __builtin_amdgcn_exp2f(__builtin_fmaf(lg, 1.44269504088896340736f, -mxl))
                                                  : expf(lg - mx);
                  s0[e & 3] += ex;
                  s1[e & 3] = __builtin_fmaf(ex, acc[kt][nt][e], s1[e & 3]);
                }
            const float t0 = (s0[0] + s0[1]) + (s0[2] + s0[3]), t1 = (s1[0] + s1[1]) + (s1[2] + s1[3]);
            score = xor32_sum(t1) / xor32_sum(t0);       // Σ softmax_k(Lg) · M  (model.py:213-214)
          } else if constexpr (SCORE == MINER_SCORE_MAX) {
            float mx = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
              for (int e = 0; e < 16; ++e)
                if (32 * kt + 16 * h + e < K) mx = fmaxf(mx, acc[kt][nt][e]);
            score = xor32_max(mx);                       // model.py:128-129
            kmx = score;
          } else {
            float sm = 0.f;
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
              for (int e = 0; e < 16; ++e)
                if (32 * kt + 16 * h + e < K) sm += acc[kt][nt][e];
            score = xor32_sum(sm) / (float)K;            // model.py:130-131
          }
          if constexpr (BIAS) if (!kRtPrior || p.bias != nullptr) score = rk_add_rn(score, pri[nt]);
          if constexpr (MODE == kCount) {
            // Lane j holds the key of target j of user uu (a slot past T: the greatest key); lanes
            // 0..31 hold the scores of news n0 + lane. The 32 score keys are broadcast in turn
            // (v_readlane) and every lane compares each with its own target — one 64-bit compare and
            // one add per (score, target) pair: T comparisons per score in one pass, whatever T (the
            // kernel is issue-bound: as three float / int compares behind a liveness branch the same
            // loop ran the config-5 call in 88.9 ms against 85.7, profiles/rk_rankof_ab.txt). A row
            // past N (a clamped copy of row N - 1), an
            // ineligible news and a NaN score take the key half 0, below every target's; a target
            // never counts itself (a key is not greater than itself). The eligibility word of
            // these 32 news is inside the bitmap whenever one of them is < N.
            const int n0 = st * kNT + 64 * nsub + 32 * nt;
            // (a scalar load: a vector load here is waited with vmcnt(0), behind the next chunk's DMAs
            // in flight, and with or without a bitmap — the wait follows the join of the branch)
            unsigned okw = 0xffffffffu;
            if (p.ok != nullptr) okw = n0 < N ? rk_sload(p.ok + __builtin_amdgcn_readfirstlane(n0 >> 5)) : 0u;
            const unsigned kh = n < N && ((okw >> r) & 1u) && score == score ? rk_okey(score) : 0u;   // 0: below every target
            const unsigned long long kt = ((unsigned long long)tg_h[uu * kMaxT + lane] << 32) | tg_l[uu * kMaxT + lane];
#pragma unroll
            for (int i = 0; i < 32; ++i) {
              const unsigned long long ki = ((unsigned long long)__builtin_amdgcn_readlane(kh, i) << 32) | rk_ikey(n0 + i);
              tcount += ki > kt ? 1 : 0;
            }
            continue;
          } else if constexpr (MODE == kPair) {
            // both uu halves hold this user's scores: the first stores (n < 0: an id outside [0, N))
            const int pos = st * kNT + 64 * nsub + 32 * nt + r;
            if (uu == 0 && h == 0 && pos < p.M) p.top_s[(size_t)ti * p.M + pos] = n >= 0 ? score : -INFINITY;
            if constexpr (INT) {
              const int g = rk_interest<NKT>(acc + (kW ? NKT : 0), nt, kmx, h, K);
              if (uu == 0 && h == 0 && pos < p.M) p.top_g[(size_t)ti * p.M + pos] = n >= 0 ? g : -1;
            }
            continue;
          }
          bool cand = h == 0 && (SUB ? n >= 0 : n < N) && user < p.U && better(score, n, th_s, th_i);
          unsigned long long bal = __ballot(cand);
          // the filters, on the few half-waves with an entry past the threshold: the eligibility
          // word of these 32 news (one per (step, nsub, nt); a candidate has n < N, so the word is
          // inside the bitmap), then the user's exclusion list, four slots per lane, against the n of
          // each candidate lane in turn (bal is wave-uniform; usually one or two bits)
          if constexpr (FLT) {
            if (bal) {
              const int n0 = st * kNT + 64 * nsub + 32 * nt;
              if constexpr (AFT) {                         // the cursor: strictly after (aft_s, aft_i)
                cand = cand && better(aft_s, aft_i, score, n);
                bal = __ballot(cand);
                if (!bal) continue;                        // (deep cursors: most half-waves end here)
              }
              if (p.ok != nullptr) {
                if constexpr (SUB) cand = cand && ((p.ok[n >> 5] >> (n & 31)) & 1u);   // per lane: ids are scattered
                else cand = cand && ((p.ok[n0 >> 5] >> r) & 1u);
                bal = __ballot(cand);
              }
              if (p.E > 0 && bal) {
                const int* ex = excl + uu * kMaxL + lane;
                const int x0 = ex[0], x1 = ex[64], x2 = ex[128], x3 = ex[192];
                unsigned long long hit = 0;
                for (unsigned long long rem = bal; rem; rem &= rem - 1) {
                  const int j = __builtin_ctzll(rem);             // lane j < 32 holds news n0 + j
                  const int nj = SUB ? __builtin_amdgcn_readlane(n, j) : n0 + j;
                  if (__ballot(x0 == nj || x1 == nj || x2 == nj || x3 == nj)) hit |= 1ull << j;
                }
                cand = cand && !((hit >> lane) & 1);
                bal &= ~hit;
              }
            }
          }
          if (bal) {
            const int buf = sl & 1;
            int b0 = 0;
            if (lane == 0) b0 = atomicAdd(&cnt[kUT + buf * kUT + uu], __popcll(bal));
            b0 = __builtin_amdgcn_readfirstlane(b0);
            // INT: the interests of this half-wave's news, only here where something is staged (bal is
            // wave-uniform, the accumulators are live, both lane halves take part in the exchange)
            [[maybe_unused]] int g = -1;
            if constexpr (INT) g = rk_interest<NKT>(acc + (kW ? NKT : 0), nt, kmx, h, K);
            if (cand) {
              const int slot = b0 + __popcll(bal & ((1ull << lane) - 1));
              stg_s[(buf * kUT + uu) * kNT + slot] = score;
              stg_i[(buf * kUT + uu) * kNT + slot] = n;
              if constexpr (INT) stg_g[(buf * kUT + uu) * kNT + slot] = g;
            }
          }
        }
      }
      // the staged candidates are merged at the next step's first chunk (merge, above), the last
      // step's below
    }
    // ---- this tile's users are done ----
    if constexpr (MODE == kCount) {
      // the four nsub waves' counts of a user, summed by its first wave; counts[user][0..T) in one
      // store. The second barrier: the next tile's targets and partial counts overwrite these.
      const int lane = fresh_lane();
      part[wave * kMaxT + lane] = tcount;
      __syncthreads();
      const int user = ti * kUT + uu;
      if (nsub == 0 && user < p.U && lane < p.T) {
        const int* pu = part + 4 * uu * kMaxT + lane;
        p.top_i[(size_t)user * p.T + lane] = (pu[0] + pu[kMaxT]) + (pu[2 * kMaxT] + pu[3 * kMaxT]);
      }
      __syncthreads();
    } else if constexpr (MODE == kRank) {   // merge the last step, write their top-k
      __syncthreads();
      if (merger && !(MINER_RK_ABL & 4)) merge((nsteps - 1) & 1);
      __syncthreads();
      const int user = ti * kUT + uu;
      if (merger && user < p.U) {
        const int lane = fresh_lane();
        const size_t o = ((size_t)user * S + slice) * p.topk;
        float* ds = S == 1 ? p.top_s : p.ws_s;
        int32_t* di = S == 1 ? p.top_i : p.ws_i;
        for (int i = lane; i < p.topk; i += 64) {
          const bool ok = i < cnt[uu];
          ds[o + i] = ok ? list_s[uu * kMaxTopk + i] : -INFINITY;
          di[o + i] = ok ? list_i[uu * kMaxTopk + i] : -1;
          if constexpr (INT) if (p.top_g != nullptr) p.top_g[o + i] = ok ? list_g[uu * kMaxTopk + i] : -1;
        }
      }
      __syncthreads();
      if (threadIdx.x < kUT) cnt[threadIdx.x] = 0;
    }
  }
}

// the S per-slice lists of a user (each best first, valid entries (id >= 0) first; the slices hold
// disjoint news, so no two entries tie in the total order) -> its top-k: an entry's rank is its
// position in its own list plus, per other list, the count of entries better than it (binary
// search); ranks < topk are written. One wave per user, its lists staged in LDS.
constexpr int kMergeUsers = 4;
__global__ __launch_bounds__(256) void rk_merge(const float* __restrict__ ws_s, const int32_t* __restrict__ ws_i, int U,
                                                int topk, float* __restrict__ top_s, int32_t* __restrict__ top_i) {
  __shared__ float ms[kMergeUsers][kSplit * kMaxTopk];
  __shared__ int mi[kMergeUsers][kSplit * kMaxTopk];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int user = blockIdx.x * kMergeUsers + w;
  if (user >= U) return;                   // wave-uniform; no block barrier below
  const size_t base = (size_t)user * kSplit * topk;
  for (int e = lane; e < kSplit * topk; e += 64) {
    ms[w][e] = ws_s[base + e];
    mi[w][e] = ws_i[base + e];
  }
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  int cnt[kSplit];
  int V = 0;
#pragma unroll
  for (int a = 0; a < kSplit; ++a) {
    int c = 0;
    for (int i0 = 0; i0 < topk; i0 += 64) c += __popcll(__ballot(i0 + lane < topk && mi[w][a * topk + i0 + lane] >= 0));
    cnt[a] = c;
    V += c;
  }
#pragma unroll
  for (int a = 0; a < kSplit; ++a) {
    for (int j = lane; j < cnt[a]; j += 64) {
      const float s = ms[w][a * topk + j];
      const int id = mi[w][a * topk + j];
      int rank = j;
#pragma unroll
      for (int o = 0; o < kSplit; ++o) {
        if (o == a) continue;
        int lo = 0, hi = cnt[o];
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (better(ms[w][o * topk + mid], mi[w][o * topk + mid], s, id)) lo = mid + 1; else hi = mid;
        }
        rank += lo;
      }
      if (rank < topk) {
        top_s[(size_t)user * topk + rank] = s;
        top_i[(size_t)user * topk + rank] = id;
      }
    }
  }
  for (int i = min(V, topk) + lane; i < topk; i += 64) {
    top_s[(size_t)user * topk + i] = -INFINITY;
    top_i[(size_t)user * topk + i] = -1;
  }
}

// Two per-user lists a [ka] and b [kb] (ka, kb <= kMaxTopk; sets of (score, id), any order, valid
// entries id >= 0) -> the first topk of their union under the ranker's total order, then the
// (-inf, -1) tail. An id in both lists keeps b's entry; with a bitmap (ok, N) entries whose id is
// at or past N or whose bit is clear drop out. One wave per user: the entries in LDS (a at slots
// [0, 256), b at [256, 512), a dropped entry's id -1), eight slots per lane, ranked by counting
// the entries better than each (equal (score, id) pairs of one list: the lower slot first, so the
// ranks are distinct whatever the input).
// CAP (a compile-time switch: the plain merge is the code it was): then the capped walk over what is
// left. The cluster ids (clus [n_clus]; an id at or past n_clus is in no cluster and no word is read
// for it) are loaded after the drop and replace steps; per entry rc = the better entries of its own
// cluster, kept iff unclustered or rc < cap; an entry's rank = the better KEPT entries; the
// (-inf, -1) tail follows the kept count.
// GM 2, the grouped merge (per-entry groups: the interests of the interest forms): an entry's group
// comes with it (a_g [U, ka] / b_g [U, kb], < 0: none) instead of from clus[id], so b's entry keeps
// b's group through the replacement; the kept entries' groups go to out_g [U, topk] (-1 in the
// tail). cap == 0: no walk, the groups are only carried.
template <int GM>
__global__ __launch_bounds__(64 * kMergeUsers) void topk_merge(const float* __restrict__ a_s, const int32_t* __restrict__ a_i,
                                                               int ka, const float* __restrict__ b_s,
                                                               const int32_t* __restrict__ b_i, int kb, int U, int topk,
                                                               const uint32_t* __restrict__ ok, int N,
                                                               float* __restrict__ out_s, int32_t* __restrict__ out_i,
                                                               const int32_t* __restrict__ clus, int n_clus, int cap,
                                                               const int32_t* __restrict__ a_g, const int32_t* __restrict__ b_g,
                                                               int32_t* __restrict__ out_g) {
  constexpr bool CAP = GM != 0, GRP = GM == 2;
  constexpr int kSlots = 2 * kMaxTopk, kPer = kSlots / 64;
  __shared__ float ms[kMergeUsers][kSlots];
  __shared__ int mi[kMergeUsers][kSlots];
  [[maybe_unused]] __shared__ int mg[CAP ? kMergeUsers : 1][CAP ? kSlots : 1];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int user = blockIdx.x * kMergeUsers + w;
  if (user >= U) return;                   // wave-uniform; no block barrier below
  float sv[kPer];
  int id[kPer];
  [[maybe_unused]] int eg[GRP ? kPer : 1];     // GRP: the groups the entries came with
#pragma unroll
  for (int t = 0; t < kPer; ++t) {
    const int e = lane + 64 * t, eb = e - kMaxTopk;
    sv[t] = -INFINITY;
    id[t] = -1;
    if constexpr (GRP) eg[t] = -1;
    if (e < ka) {
      sv[t] = a_s[(size_t)user * ka + e];
      id[t] = a_i[(size_t)user * ka + e];
      if constexpr (GRP) eg[t] = max(a_g[(size_t)user * ka + e], -1);
    } else if (eb >= 0 && eb < kb) {
      sv[t] = b_s[(size_t)user * kb + eb];
      id[t] = b_i[(size_t)user * kb + eb];
      if constexpr (GRP) eg[t] = max(b_g[(size_t)user * kb + eb], -1);
    }
    if (ok != nullptr && id[t] >= 0 && (id[t] >= N || !((ok[id[t] >> 5] >> (id[t] & 31)) & 1u))) id[t] = -1;
    if (id[t] < 0) id[t] = -1;
    mi[w][e] = id[t];
  }
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  // an entry of a whose id b holds gives way to b's
  for (int j = 0; j < kb; ++j) {
    const int bj = mi[w][kMaxTopk + j];
#pragma unroll
    for (int t = 0; t < kMaxTopk / 64; ++t)
      if (bj >= 0 && id[t] == bj) id[t] = -1;
  }
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int t = 0; t < kPer; ++t) {
    ms[w][lane + 64 * t] = sv[t];
    mi[w][lane + 64 * t] = id[t];
  }
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  if constexpr (CAP) {
    // the cap: an entry with cap or more better entries of its own cluster leaves (its id becomes
    // -1, as a pruned entry's), then the ranking below runs over the kept entries alone
    int g[kPer], rc[kPer];
#pragma unroll
    for (int t = 0; t < kPer; ++t) {
      if constexpr (GRP) g[t] = id[t] >= 0 ? eg[t] : -1;
      else g[t] = id[t] >= 0 && id[t] < n_clus ? max(clus[id[t]], -1) : -1;
      mg[w][lane + 64 * t] = g[t];
      rc[t] = 0;
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    for (int half = 0; half < 2 && (!GRP || cap > 0); ++half) {
      const int j0 = half * kMaxTopk, j1 = j0 + (half ? kb : ka);
      for (int j = j0; j < j1; ++j) {
        const int i2 = mi[w][j], g2 = mg[w][j];
        if (i2 < 0 || g2 < 0) continue;      // wave-uniform
        const float s2 = ms[w][j];
#pragma unroll
        for (int t = 0; t < kPer; ++t)
          rc[t] += g[t] == g2 && (better(s2, i2, sv[t], id[t]) || (s2 == sv[t] && i2 == id[t] && j < lane + 64 * t)) ? 1 : 0;
      }
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();          // every read of the ids comes before the first write
#pragma unroll
    for (int t = 0; t < kPer; ++t) {
      if (g[t] >= 0 && rc[t] >= cap && (!GRP || cap > 0)) {
        id[t] = -1;
        mi[w][lane + 64 * t] = -1;
      }
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
  }
  int rank[kPer];
#pragma unroll
  for (int t = 0; t < kPer; ++t) rank[t] = 0;
  for (int half = 0; half < 2; ++half) {
    const int j0 = half * kMaxTopk, j1 = j0 + (half ? kb : ka);
    for (int j = j0; j < j1; ++j) {
      const float s2 = ms[w][j];
      const int i2 = mi[w][j];
      if (i2 < 0) continue;                // wave-uniform
#pragma unroll
      for (int t = 0; t < kPer; ++t)
        rank[t] += better(s2, i2, sv[t], id[t]) || (s2 == sv[t] && i2 == id[t] && j < lane + 64 * t) ? 1 : 0;
    }
  }
  int V = 0;
#pragma unroll
  for (int t = 0; t < kPer; ++t) {
    V += __popcll(__ballot(id[t] >= 0));
    if (id[t] >= 0 && rank[t] < topk) {
      out_s[(size_t)user * topk + rank[t]] = sv[t];
      out_i[(size_t)user * topk + rank[t]] = id[t];
      if constexpr (GRP) out_g[(size_t)user * topk + rank[t]] = eg[t];
    }
  }
  for (int i = min(V, topk) + lane; i < topk; i += 64) {
    out_s[(size_t)user * topk + i] = -INFINITY;
    out_i[(size_t)user * topk + i] = -1;
    if constexpr (GRP) out_g[(size_t)user * topk + i] = -1;
  }
}

// The state of a resumed capped walk advanced by one served page, one wave per user: the cursor that
// continues the page (page_cursor's rule: the row's last entry if it is full, else (-inf, 2^31 - 1))
// and the union of the served-group table with the groups of the page's entries, counts summed,
// strictly ascending. An entry's group is pg[u][j] when given, else clus[id] for an id inside
// [0, n_clus); an entry with id < 0 or a negative group adds nothing. The in table is ascending and
// distinct (the precondition), so only the page is ranked by counting: a page entry leads its group
// if no earlier entry of the page has it; a leader found in the in table (binary search, in LDS) adds
// its multiplicity to that pair, a new leader goes to (the in pairs below it) + (the new leaders below
// it), and an in pair moves up by the new leaders below it. More than Q pairs: overflow[u] = 1, the
// cursor becomes "after everything" (the walk ends rather than ever breaking a cap) and the Q lowest
// groups are written. Every LDS write is followed by a wave barrier before it is read.
constexpr int kMaxWalk = MINER_CORPUS_MAX_WALK_GROUPS;
__global__ __launch_bounds__(64 * kMergeUsers) void walk_advance(const float* __restrict__ ps, const int32_t* __restrict__ pi,
                                                                 const int32_t* __restrict__ pg,
                                                                 const int32_t* __restrict__ clus, int n_clus,
                                                                 const int32_t* __restrict__ in_g,
                                                                 const int32_t* __restrict__ in_c,
                                                                 const int32_t* __restrict__ in_n, int Qin,
                                                                 float* __restrict__ out_as, int32_t* __restrict__ out_ai,
                                                                 int32_t* __restrict__ out_g, int32_t* __restrict__ out_c,
                                                                 int32_t* __restrict__ out_n, uint8_t* __restrict__ overflow,
                                                                 int U, int k, int Q) {
  constexpr int kPT = kMaxTopk / 64, kQT = kMaxWalk / 64;
  __shared__ int tg[kMergeUsers][kMaxWalk];     // the in table's groups
  __shared__ int ta[kMergeUsers][kMaxWalk];     // what the page adds to each in pair
  __shared__ int eg[kMergeUsers][kMaxTopk];     // the page entries' groups (-1: none), then -1 unless a NEW leader
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int user = blockIdx.x * kMergeUsers + w;
  if (user >= U) return;                   // wave-uniform; no block barrier below
  const int nin = Qin > 0 ? min(max(in_n[user], 0), Qin) : 0;
  int g[kPT], mult[kPT];
  bool lead[kPT];
#pragma unroll
  for (int t = 0; t < kPT; ++t) {
    const int j = lane + 64 * t;
    g[t] = -1;
    if (j < k) {
      const int id = pi[(size_t)user * k + j];
      if (id >= 0) {
        if (pg != nullptr) g[t] = max(pg[(size_t)user * k + j], -1);
        else if (id < n_clus) g[t] = max(clus[id], -1);
      }
    }
    eg[w][j] = g[t];
    mult[t] = 0;
    lead[t] = g[t] >= 0;
  }
#pragma unroll
  for (int q = 0; q < kQT; ++q) {
    const int i = lane + 64 * q;
    tg[w][i] = i < nin ? in_g[(size_t)user * Qin + i] : 0x7fffffff;
    ta[w][i] = 0;
  }
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  // a page entry's multiplicity and whether it leads its group
  for (int j2 = 0; j2 < k; ++j2) {
    const int g2 = eg[w][j2];
    if (g2 < 0) continue;                  // wave-uniform
#pragma unroll
    for (int t = 0; t < kPT; ++t) {
      mult[t] += g[t] == g2 ? 1 : 0;
      if (g[t] == g2 && j2 < lane + 64 * t) lead[t] = false;
    }
  }
  // a leader's lower bound in the in table: found -> it adds to that pair; else a new group
  int below[kPT];
  bool fresh[kPT];
#pragma unroll
  for (int t = 0; t < kPT; ++t) {
    int lo = 0, hi = nin;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (tg[w][mid] < g[t]) lo = mid + 1; else hi = mid;
    }
    below[t] = lo;
    const bool found = lead[t] && lo < nin && tg[w][lo] == g[t];
    fresh[t] = lead[t] && !found;
    if (found) ta[w][lo] = mult[t];        // one leader per group: no two lanes write one slot
  }
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();          // every read of the page groups comes before this rewrite
#pragma unroll
  for (int t = 0; t < kPT; ++t) eg[w][lane + 64 * t] = fresh[t] ? g[t] : -1;
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  // positions: the new leaders below each new leader and below each in pair
  int ig[kQT], up[kQT], nb[kPT];
#pragma unroll
  for (int q = 0; q < kQT; ++q) { ig[q] = tg[w][lane + 64 * q]; up[q] = 0; }
#pragma unroll
  for (int t = 0; t < kPT; ++t) nb[t] = 0;
  int nnew = 0;
  for (int j2 = 0; j2 < k; ++j2) {
    const int g2 = eg[w][j2];
    if (g2 < 0) continue;                  // wave-uniform
    ++nnew;
#pragma unroll
    for (int t = 0; t < kPT; ++t) nb[t] += g2 < g[t] ? 1 : 0;
#pragma unroll
    for (int q = 0; q < kQT; ++q) up[q] += g2 < ig[q] ? 1 : 0;
  }
  const int total = nin + nnew;
  const bool over = total > Q;
#pragma unroll
  for (int q = 0; q < kQT; ++q) {
    const int i = lane + 64 * q, pos = i + up[q];
    if (i < nin && pos < Q) {
      out_g[(size_t)user * Q + pos] = ig[q];
      out_c[(size_t)user * Q + pos] = max(in_c[(size_t)user * Qin + i], 0) + ta[w][i];
    }
  }
#pragma unroll
  for (int t = 0; t < kPT; ++t) {
    const int pos = below[t] + nb[t];
    if (fresh[t] && pos < Q) {
      out_g[(size_t)user * Q + pos] = g[t];
      out_c[(size_t)user * Q + pos] = mult[t];
    }
  }
  if (lane == 0) {
    const int last = pi[(size_t)user * k + k - 1];
    const bool full = last >= 0 && !over;
    out_as[user] = full ? ps[(size_t)user * k + k - 1] : -INFINITY;
    out_ai[user] = full ? last : 0x7fffffff;
    out_n[user] = min(total, Q);
    overflow[user] = over ? 1 : 0;
  }
}

// every list empty: (-inf, -1) (the subset form with an empty id list)
__global__ __launch_bounds__(256) void rk_fill_empty(float* __restrict__ top_s, int32_t* __restrict__ top_i,
                                                     int32_t* __restrict__ top_g, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    top_s[i] = -INFINITY;
    top_i[i] = -1;
    if (top_g != nullptr) top_g[i] = -1;
  }
}

// ================================================================================================
// host side
// ================================================================================================
bool dtype_ok(int dt) { return dt == MINER_DTYPE_F32 || dt == MINER_DTYPE_BF16 || dt == MINER_DTYPE_F16; }
size_t esize(int dt) { return dt == MINER_DTYPE_F32 ? 4 : 2; }

template <class T, int NKT, bool G>
int ue_launch(void* stream, const UeParams& prm) {
  auto kern = ue_fused<T, NKT, G>;
  const int lds = kUeLds<T>;
  hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e != hipSuccess) return (int)e;
  int grid = num_cus();
  if (grid > prm.U) grid = prm.U;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kThreads), lds, static_cast<hipStream_t>(stream), prm);
  e = hipGetLastError();
  return e == hipSuccess ? MINER_OK : (int)e;
}

template <class T>
int ue_dispatch(void* stream, const UeParams& prm) {
  const bool g = prm.his_ids != nullptr;
  if (prm.K <= 32) return g ? ue_launch<T, 1, true>(stream, prm) : ue_launch<T, 1, false>(stream, prm);
  return g ? ue_launch<T, 2, true>(stream, prm) : ue_launch<T, 2, false>(stream, prm);
}

// the split form (S = kSplit news slices, rk_merge) when the caller gave a workspace, the device has
// the 256 CUs its tile-to-XCD map assumes, and the users are too few to fill the CUs with 2-user
// tiles (< 256 two-user tiles, i.e. U <= 510): at U = 2,048 it measured 90.5 vs 85.9 ms per config-5 step (each slice's
// top-k warms up on its own; its L2 hit rate is higher, 69 vs 45 %, but the stream is not what
// bounds it). The caller chooses by passing a workspace (miner_rank_topk_split_recommended says
// which form the library would take). Fewer than 256 two-user tiles means U <= 510.
bool rk_split_wanted(int U) { return num_cus() == 256 && (U + kUT - 1) / kUT < num_cus(); }
size_t rk_ws_bytes(int U, int topk) { return (size_t)U * kSplit * topk * 8; }
// the split form runs only on a workspace whose stated size covers it (the launch never trusts an
// earlier size query), on the 256-CU device its tile-to-XCD map assumes
bool rk_split(const RkParams& prm) {
  if (prm.ws_s == nullptr || prm.ws_i == nullptr || prm.ws_bytes < rk_ws_bytes(prm.U, prm.topk)) return false;
  return num_cus() == 256;
}

// The forms the library launches: the table below, and rk_form, the one rule that maps a call to
// its entry. Every feature is a compile-time switch so that a call without it launches the code it
// launched before the feature existed (the measured costs of run-time tests: the switches above).
constexpr unsigned kFSubset = kFFlt | kFSub;       // the subset form: filtered (either filter may be null)
constexpr unsigned kFBiased = kFFlt | kFBias;      // the biased ranking forms: filtered (as the subset form), GEO 0
constexpr unsigned kFCursor = kFBiased | kFAft;    // the cursor form: on the biased form, the prior tested at run time
constexpr unsigned kFCapped = kFBiased | kFCap;    // the capped form: on the biased form likewise, unsplit
constexpr unsigned kFPairs = kFPair | kFSubset;    // the pair form gathers: SUB (and so FLT)
constexpr unsigned kRkForms[] = {
    0, kFFlt, kFSubset, kFBiased, kFBiased | kFSub, kFCursor, kFCursor | kFSub,
    kFSplit, kFSplit | kFFlt, kFSplit | kFSubset, kFSplit | kFBiased, kFSplit | kFBiased | kFSub, kFSplit | kFCursor,
    kFSplit | kFCursor | kFSub,
    kFCapped, kFCapped | kFSub, kFCount, kFCount | kFBias, kFPairs, kFPairs | kFBias,
    // the interest forms (never instantiated for the mean score: rk_pick)
    kFPairs | kFInt, kFPairs | kFBias | kFInt, kFCapped | kFInt, kFCapped | kFSub | kFInt,
    // the resumed capped walks: the capped forms with the cursor and the served-group table
    kFCapped | kFAft, kFCapped | kFAft | kFSub, kFCapped | kFAft | kFInt, kFCapped | kFAft | kFSub | kFInt,
#ifdef MINER_RK_GEO1
    kFGeo1, kFGeo1 | kFFlt, kFGeo1 | kFSplit, kFGeo1 | kFSplit | kFFlt,
#endif
};

unsigned rk_form(const RkParams& prm, int mode, [[maybe_unused]] int dtype) {
  // the counting and pair forms: unsplit, GEO 0; the biased instantiation only when a prior table
  // was given (the unbiased calls launch what they did)
  if (mode == kCount) return kFCount | (prm.bias != nullptr ? kFBias : 0);
  // (the interest instantiation only when the interests were asked for)
  if (mode == kPair) return kFPairs | (prm.bias != nullptr ? kFBias : 0) | (prm.top_g != nullptr ? kFInt : 0);
  // the id list: one instantiation per shape of every form below, table or subset
  const unsigned sub = prm.ids != nullptr ? kFSub : 0;
  // the capped form — two kernels per shape (table / subset), not four. A workspace is never written.
  // (the resumed instantiation only with a served-group table: a capped call without one launches what it did)
  const unsigned res = prm.use_g != nullptr ? kFAft : 0;
  if (prm.clus != nullptr) return kFCapped | sub | res;
  // the interest-capped form: the capped form with the group taken from the epilogue
  if (prm.icap > 0) return kFCapped | kFInt | sub | res;
  const unsigned split = rk_split(prm) ? kFSplit : 0;
  if (prm.aft_s != nullptr) return kFCursor | sub | split;
  if (prm.bias != nullptr) return kFBiased | sub | split;
  if (sub) return kFSubset | split;
  const unsigned flt = prm.ok != nullptr || prm.E > 0 ? kFFlt : 0;     // the filtered instantiation only when asked for
  // (GEO 1 — 64-byte rows through a 4-stage ring, three chunks in flight instead of one — measured
  // slower: 95.9 vs 89.7 ms per config-5 step, twice the barriers for no gain in the gather rate;
  // diagnostic builds with -DMINER_RK_GEO1 launch it, in 16-bit with at least two row tiles per user)
#ifdef MINER_RK_GEO1
  if (dtype != MINER_DTYPE_F32 && (prm.K > 32 || prm.score_type == MINER_SCORE_WEIGHTED)) return kFGeo1 | flt | split;
#endif
  return flt | split;
}

// the one launcher: form F of the table with the compile-time shape added — in 16-bit config 5's
// d = 768 as the chunk count and, on two interest tiles, its K = 64 (the masked interest loops of
// the epilogue compile away; the top-k equals the oracle's at the 16-bit bar, tests/test_gpu_corpus.py).
// Every form takes its shape by this rule, so a pair's score has the bits of the ranking form that
// the same shape launches.
template <class T, int NKT, int SCORE, unsigned F0>
int rk_launch(void* stream, const RkParams& prm) {
  constexpr int NR = SCORE == MINER_SCORE_WEIGHTED ? 2 * NKT : NKT;
  constexpr unsigned F = sizeof(T) == 2 && NR >= 2 ? F0 : F0 & ~kFGeo1;   // (rk_form asks for GEO 1 nowhere else)
  using Fm = RkForm<F>;
  void (*kern)(RkParams) = rk_fused<T, NKT, SCORE, F>;
  if constexpr (sizeof(T) == 2) {
    if (prm.d == 768) {
      kern = rk_fused<T, NKT, SCORE, F | kFD768>;
      if constexpr (NKT == 2)
        if (prm.K == 64) kern = rk_fused<T, NKT, SCORE, F | kFD768 | kFK64>;
    }
  }
  constexpr int lds = RkLds<NR, Fm::GEO, Fm::FLT, Fm::CAP, Fm::INT>::kTotal;
  static_assert(lds <= 160 * 1024, "ranker LDS (with the exclusion lists and the cluster ids of the form)");
  hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e != hipSuccess) return (int)e;
  constexpr bool split = Fm::S > 1;
  const int ntiles = Fm::MODE == kPair ? prm.U : (prm.U + kUT - 1) / kUT;   // pair form: a tile is one user
  int grid = num_cus();
  if (!split && grid > ntiles) grid = ntiles;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kThreads), lds, s, prm);
  e = hipGetLastError();
  if (e != hipSuccess || !split) return e == hipSuccess ? MINER_OK : (int)e;
  hipLaunchKernelGGL(rk_merge, dim3((prm.U + kMergeUsers - 1) / kMergeUsers), dim3(64 * kMergeUsers), 0, s, prm.ws_s,
                     prm.ws_i, prm.U, prm.topk, prm.top_s, prm.top_i);
  e = hipGetLastError();
  return e == hipSuccess ? MINER_OK : (int)e;
}

// (the mean score has no dominant interest: its interest forms do not exist, and the entry points
// have answered MINER_EINVAL before anything gets here)
template <class T, int NKT, int SCORE, unsigned F>
int rk_launch_form(void* stream, const RkParams& prm) {
  if constexpr (SCORE == MINER_SCORE_MEAN && (F & kFInt) != 0) return MINER_EINVAL;
  else return rk_launch<T, NKT, SCORE, F>(stream, prm);
}

// the one ladder, for every mode: dtype, K <= 32 (one interest tile), score type, then the table
template <class T, int NKT, int SCORE, size_t... I>
int rk_pick(void* stream, const RkParams& prm, unsigned form, std::index_sequence<I...>) {
  int rc = MINER_EINVAL;
  (void)((form == kRkForms[I] && ((rc = rk_launch_form<T, NKT, SCORE, kRkForms[I]>(stream, prm)), true)) || ...);
  return rc;
}
template <class T, int NKT>
int rk_by_score(void* stream, const RkParams& prm, unsigned form) {
  constexpr std::make_index_sequence<sizeof(kRkForms) / sizeof(kRkForms[0])> all{};
  if (prm.score_type == MINER_SCORE_WEIGHTED) return rk_pick<T, NKT, MINER_SCORE_WEIGHTED>(stream, prm, form, all);
  if (prm.score_type == MINER_SCORE_MAX) return rk_pick<T, NKT, MINER_SCORE_MAX>(stream, prm, form, all);
  return rk_pick<T, NKT, MINER_SCORE_MEAN>(stream, prm, form, all);
}
template <class T>
int rk_by_k(void* stream, const RkParams& prm, unsigned form) {
  return prm.K <= 32 ? rk_by_score<T, 1>(stream, prm, form) : rk_by_score<T, 2>(stream, prm, form);
}
int rk_dispatch(void* stream, int dtype, const RkParams& prm, int mode) {
  const unsigned form = rk_form(prm, mode, dtype);
  if (dtype == MINER_DTYPE_BF16) return rk_by_k<__bf16>(stream, prm, form);
  if (dtype == MINER_DTYPE_F16) return rk_by_k<_Float16>(stream, prm, form);
  return rk_by_k<float>(stream, prm, form);
}

int check_dims(int dtype, int d, int Dc, int K) {
  if (!dtype_ok(dtype) || d <= 0 || K <= 0 || Dc <= 0) return MINER_EINVAL;
  if (K > kMaxK || Dc > 32 * kDcT || d > kMaxD) return MINER_ESHAPE;
  if (d % (dtype == MINER_DTYPE_F32 ? 32 : 64)) return MINER_ESHAPE;
  return MINER_OK;
}

// the prior table's checks, shared by the three biased entry points (after each one's own); G and
// the group ids are read only with a table
int bias_check(RkParams& prm) {
  if (prm.bias != nullptr && prm.G <= 0) return MINER_EINVAL;
  if (prm.bias == nullptr && prm.grp != nullptr) return MINER_EINVAL;
  if (!aligned4(prm.bias)) return MINER_EALIGN;
  if (!aligned4(prm.grp)) return MINER_EALIGN;
  if (prm.bias == nullptr) prm.G = 0;
  return MINER_OK;
}

// the cluster table's checks, shared by the two capped entry points (after each one's own); cap is
// read only with a table
int cap_check(const int32_t* news_cluster, int cap) {
  if (news_cluster != nullptr && cap <= 0) return MINER_EINVAL;
  if (news_cluster != nullptr && cap > kMaxTopk) return MINER_ESHAPE;
  return MINER_OK;
}

// the checks every entry point of the ranker starts with, on its arguments as prm holds them; the
// list entries (rank) also answer for topk and the two list outputs, at their places in the order
int rk_check_common(int dtype, const RkParams& prm, bool rank) {
  const int ck = check_dims(dtype, prm.d, 1, prm.K);
  if (ck != MINER_OK) return ck;
  if (prm.score_type < MINER_SCORE_WEIGHTED || prm.score_type > MINER_SCORE_MEAN) return MINER_EINVAL;
  if (prm.U < 0 || prm.N <= 0 || (rank && prm.topk <= 0)) return MINER_EINVAL;
  if (rank && prm.topk > kMaxTopk) return MINER_ESHAPE;
  if (!prm.mui || !prm.news || (rank && (!prm.top_s || !prm.top_i))) return MINER_EINVAL;
  if (prm.score_type == MINER_SCORE_WEIGHTED && !prm.proj) return MINER_EINVAL;
  if (!aligned16(prm.mui) || !aligned16(prm.proj) || !aligned16(prm.news)) return MINER_EALIGN;
  return MINER_OK;
}

// every miner_rank_topk* entry point: prm holds the arguments as the caller gave them (the widest
// entry's; the whole table is a NULL id list with M < 0); what a feature left NULL does not read is
// cleared once the checks have passed. The id list's checks follow the table forms' checks, which
// keep their order and codes.
int rk_run(void* stream, int dtype, RkParams prm, void* workspace, size_t workspace_bytes) {
  const int ck = rk_check_common(dtype, prm, true);
  if (ck != MINER_OK) return ck;
  if (prm.E < 0 || (prm.E > 0 && !prm.excl)) return MINER_EINVAL;
  if (prm.E > kMaxL) return MINER_ESHAPE;
  if (!aligned4(prm.excl) || !aligned4(prm.ok)) return MINER_EALIGN;
  const bool subset = prm.ids != nullptr || prm.M >= 0;
  if (subset) {
    if (prm.M < 0 || (prm.M > 0 && !prm.ids)) return MINER_EINVAL;
    if (!aligned4(prm.ids)) return MINER_EALIGN;
  }
  const int bk = bias_check(prm);
  if (bk != MINER_OK) return bk;
  const int cc = cap_check(prm.clus, prm.cap);
  if (cc != MINER_OK) return cc;
  if (!aligned4(prm.clus)) return MINER_EALIGN;
  // the cursor: both words or neither, never with caps (a capped walk also needs the earlier pages'
  // per-cluster counts, which a (score, id) pair does not carry)
  // (a served-group table — miner_rank_topk_resume — carries those counts and lifts the refusal)
  const bool resume = prm.use_g != nullptr || prm.use_c != nullptr || prm.use_n != nullptr;
  if ((prm.aft_s == nullptr) != (prm.aft_i == nullptr)) return MINER_EINVAL;
  if (prm.aft_s != nullptr && prm.clus != nullptr && !resume) return MINER_EINVAL;
  if (!aligned4(prm.aft_s) || !aligned4(prm.aft_i)) return MINER_EALIGN;
  // the per-interest cap: the capped form's restrictions (no cluster table beside it, no cursor), a
  // score type that has a dominant interest, and the interests out only under a cap
  if (prm.icap < 0) return MINER_EINVAL;
  if (prm.icap > kMaxTopk) return MINER_ESHAPE;
  if (prm.icap > 0 && (prm.clus != nullptr || (prm.aft_s != nullptr && !resume))) return MINER_EINVAL;
  if (prm.icap > 0 && prm.score_type == MINER_SCORE_MEAN) return MINER_EINVAL;
  if (prm.icap == 0 && prm.top_g != nullptr) return MINER_EINVAL;
  if (!aligned4(prm.top_g)) return MINER_EALIGN;
  // the resumed walk: a cursor, exactly one kind of cap (both at once has answered above), the whole
  // table triple, its capacity and alignment
  if (resume) {
    if (prm.aft_s == nullptr) return MINER_EINVAL;
    if (prm.clus == nullptr && prm.icap == 0) return MINER_EINVAL;
    if (prm.Q < 0 || prm.use_g == nullptr || prm.use_c == nullptr || prm.use_n == nullptr) return MINER_EINVAL;
    if (prm.Q > MINER_CORPUS_MAX_WALK_GROUPS) return MINER_ESHAPE;
    if (!aligned4(prm.use_g) || !aligned4(prm.use_c) || !aligned4(prm.use_n)) return MINER_EALIGN;
  }
  if (prm.U == 0) return MINER_OK;
  if (!aligned16(workspace)) return MINER_EALIGN;
  if (subset && prm.M == 0) {              // nothing to rank: every list empty, no ranker launch
    const size_t n = (size_t)prm.U * prm.topk;
    hipLaunchKernelGGL(rk_fill_empty, dim3((unsigned)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), prm.top_s, prm.top_i, prm.top_g, n);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MINER_OK : (int)e;
  }
  if (workspace) {
    prm.ws_bytes = workspace_bytes;
    prm.ws_s = static_cast<float*>(workspace);
    prm.ws_i = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + (size_t)prm.U * kSplit * prm.topk * 4);
  }
  if (prm.E == 0) prm.excl = nullptr;
  if (!subset) { prm.ids = nullptr; prm.M = 0; }
  if (prm.clus == nullptr) prm.cap = prm.icap;       // (0 without either kind of cap)
  return rk_dispatch(stream, dtype, prm, kRank);
}

// the fields every miner_rank_topk* entry point has; each entry sets what it adds by name. M = -1:
// the whole table (a NULL id list)
RkParams rk_params(int score_type, const void* user_mui, const void* user_proj, const void* news, int U, int N, int d, int K,
                   int topk, float* top_scores, int32_t* top_ids) {
  RkParams prm{};
  prm.mui = user_mui; prm.proj = user_proj; prm.news = news; prm.top_s = top_scores; prm.top_i = top_ids;
  prm.U = U; prm.N = N; prm.d = d; prm.K = K; prm.topk = topk; prm.score_type = score_type;
  prm.M = -1;
  return prm;
}

// every miner_score_pairs* entry point: the pairs are prm.ids [U][M], the scores go to prm.top_s and
// the interests (NULL: not wanted) to prm.top_g
int pair_run(void* stream, int dtype, RkParams prm) {
  const int ck = rk_check_common(dtype, prm, false);
  if (ck != MINER_OK) return ck;
  if (prm.M < 0 || (prm.M > 0 && (!prm.ids || !prm.top_s))) return MINER_EINVAL;
  if (!aligned4(prm.ids) || !aligned4(prm.top_s)) return MINER_EALIGN;
  const int bk = bias_check(prm);
  if (bk != MINER_OK) return bk;
  // the interests: a score type that has a dominant interest, then the alignment
  if (prm.top_g != nullptr && prm.score_type == MINER_SCORE_MEAN) return MINER_EINVAL;
  if (!aligned4(prm.top_g)) return MINER_EALIGN;
  if (prm.U == 0 || prm.M == 0) return MINER_OK;
  return rk_dispatch(stream, dtype, prm, kPair);
}

// both miner_rank_count* entry points: the counts go to prm.top_i [U][T]
int count_run(void* stream, int dtype, RkParams prm) {
  const int ck = rk_check_common(dtype, prm, false);
  if (ck != MINER_OK) return ck;
  if (prm.T <= 0 || !prm.tgt_s || !prm.tgt_i || !prm.top_i) return MINER_EINVAL;
  if (prm.T > kMaxT) return MINER_ESHAPE;
  if (!aligned4(prm.tgt_s) || !aligned4(prm.tgt_i) || !aligned4(prm.ok) || !aligned4(prm.top_i)) return MINER_EALIGN;
  const int bk = bias_check(prm);
  if (bk != MINER_OK) return bk;
  if (prm.U == 0) return MINER_OK;
  return rk_dispatch(stream, dtype, prm, kCount);
}

// the checks the list-merge entry points start with, and their one launch
int merge_check(const float* a_scores, const int32_t* a_ids, int ka, const float* b_scores, const int32_t* b_ids, int kb,
                int U, int topk, const uint32_t* news_ok, int N, float* out_scores, int32_t* out_ids) {
  if (U < 0 || ka < 0 || kb < 0 || topk <= 0) return MINER_EINVAL;
  if (ka > kMaxTopk || kb > kMaxTopk || topk > kMaxTopk) return MINER_ESHAPE;
  if ((ka > 0 && (!a_scores || !a_ids)) || (kb > 0 && (!b_scores || !b_ids)) || !out_scores || !out_ids) return MINER_EINVAL;
  if (news_ok && N <= 0) return MINER_EINVAL;
  if (!aligned4(a_scores) || !aligned4(a_ids) || !aligned4(b_scores) || !aligned4(b_ids) || !aligned4(news_ok) ||
      !aligned4(out_scores) || !aligned4(out_ids))
    return MINER_EALIGN;
  return MINER_OK;
}
using MergeKernel = void (*)(const float*, const int32_t*, int, const float*, const int32_t*, int, int, int, const uint32_t*,
                             int, float*, int32_t*, const int32_t*, int, int, const int32_t*, const int32_t*, int32_t*);
int merge_launch(MergeKernel kern, void* stream, const float* a_scores, const int32_t* a_ids, int ka, const float* b_scores,
                 const int32_t* b_ids, int kb, int U, int topk, const uint32_t* news_ok, int N, float* out_scores,
                 int32_t* out_ids, const int32_t* clus, int n_clus, int cap, const int32_t* a_groups,
                 const int32_t* b_groups, int32_t* out_groups) {
  hipLaunchKernelGGL(kern, dim3((U + kMergeUsers - 1) / kMergeUsers), dim3(64 * kMergeUsers), 0,
                     static_cast<hipStream_t>(stream), a_scores, a_ids, ka, b_scores, b_ids, kb, U, topk, news_ok, N,
                     out_scores, out_ids, clus, n_clus, cap, a_groups, b_groups, out_groups);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MINER_OK : (int)e;
}

}  // namespace

extern "C" {

int miner_score_pairs(void* stream, int dtype, int score_type, const void* user_mui, const void* user_proj,
                      const void* news, int U, int N, int d, int K, const int32_t* cand_ids, int C, float* scores) {
  RkParams prm = rk_params(score_type, user_mui, user_proj, news, U, N, d, K, 0, scores, nullptr);
  prm.ids = cand_ids; prm.M = C;
  return pair_run(stream, dtype, prm);
}

int miner_score_pairs_biased(void* stream, int dtype, int score_type, const void* user_mui, const void* user_proj,
                             const void* news, int U, int N, int d, int K, const int32_t* cand_ids, int C, float* scores,
                             const float* news_bias, int G, const int32_t* user_group) {
  RkParams prm = rk_params(score_type, user_mui, user_proj, news, U, N, d, K, 0, scores, nullptr);
  prm.ids = cand_ids; prm.M = C;
  prm.bias = news_bias; prm.G = G; prm.grp = user_group;
  return pair_run(stream, dtype, prm);
}

int miner_score_pairs_interest(void* stream, int dtype, int score_type, const void* user_mui, const void* user_proj,
                               const void* news, int U, int N, int d, int K, const int32_t* cand_ids, int C, float* scores,
                               const float* news_bias, int G, const int32_t* user_group, int32_t* interests) {
  RkParams prm = rk_params(score_type, user_mui, user_proj, news, U, N, d, K, 0, scores, nullptr);
  prm.ids = cand_ids; prm.M = C;
  prm.bias = news_bias; prm.G = G; prm.grp = user_group;
  prm.top_g = interests;
  return pair_run(stream, dtype, prm);
}

int miner_rank_count(void* stream, int dtype, int score_type, const void* user_mui, const void* user_proj,
                     const void* news, int U, int N, int d, int K, const float* target_scores, const int32_t* target_ids,
                     int T, const uint32_t* news_ok, int32_t* counts) {
  RkParams prm = rk_params(score_type, user_mui, user_proj, news, U, N, d, K, 0, nullptr, counts);
  prm.M = 0;
  prm.ok = news_ok; prm.tgt_s = target_scores; prm.tgt_i = target_ids; prm.T = T;
  return count_run(stream, dtype, prm);
}

int miner_rank_count_biased(void* stream, int dtype, int score_type, const void* user_mui, const void* user_proj,
                            const void* news, int U, int N, int d, int K, const float* target_scores,
                            const int32_t* target_ids, int T, const uint32_t* news_ok, int32_t* counts,
                            const float* news_bias, int G, const int32_t* user_group) {
  RkParams prm = rk_params(score_type, user_mui, user_proj, news, U, N, d, K, 0, nullptr, counts);
  prm.M = 0;
  prm.ok = news_ok; prm.tgt_s = target_scores; prm.tgt_i = target_ids; prm.T = T;
  prm.bias = news_bias; prm.G = G; prm.grp = user_group;
  return count_run(stream, dtype, prm);
}

size_t miner_encoder_packed_bytes(int dtype, int d, int Dc, int K) {
  if (check_dims(dtype, d, Dc, K) != MINER_OK) return 0;
  return (ue_w1_elems(d) + ue_q_elems(K) + ue_w2_elems(d)) * esize(dtype);
}

int miner_encoder_pack(void* stream, int dtype, const void* w_poly, const void* context_codes, const void* w_target,
                       int d, int Dc, int K, void* packed) {
  const int ck = check_dims(dtype, d, Dc, K);
  if (ck != MINER_OK) return ck;
  if (!w_poly || !context_codes || !packed) return MINER_EINVAL;
  if (!aligned16(packed)) return MINER_EALIGN;
  const size_t n = ue_w1_elems(d) + ue_q_elems(K) + (w_target ? ue_w2_elems(d) : 0);
  const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == MINER_DTYPE_BF16)
    hipLaunchKernelGGL(ue_pack_kernel<__bf16>, dim3(grid), dim3(256), 0, s, static_cast<const __bf16*>(w_poly),
                       static_cast<const __bf16*>(context_codes), static_cast<const __bf16*>(w_target), d, Dc, K,
                       static_cast<__bf16*>(packed));
  else if (dtype == MINER_DTYPE_F16)
    hipLaunchKernelGGL(ue_pack_kernel<_Float16>, dim3(grid), dim3(256), 0, s, static_cast<const _Float16*>(w_poly),
                       static_cast<const _Float16*>(context_codes), static_cast<const _Float16*>(w_target), d, Dc, K,
                       static_cast<_Float16*>(packed));
  else
    hipLaunchKernelGGL(ue_pack_kernel<float>, dim3(grid), dim3(256), 0, s, static_cast<const float*>(w_poly),
                       static_cast<const float*>(context_codes), static_cast<const float*>(w_target), d, Dc, K,
                       static_cast<float*>(packed));
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MINER_OK : (int)e;
}

int miner_encode_users(void* stream, int dtype, const void* history, const int32_t* his_ids, int n_news,
                       const uint8_t* his_mask, const float* his_bias, const void* packed, int U, int L, int d,
                       int Dc, int K, float* mui_f32, void* user_mui, void* user_proj) {
  const int ck = check_dims(dtype, d, Dc, K);
  if (ck != MINER_OK) return ck;
  if (U < 0 || L <= 0) return MINER_EINVAL;
  if (L > kMaxL) return MINER_ESHAPE;
  if (!history || !his_mask || !packed || !user_mui) return MINER_EINVAL;
  if (his_ids && n_news <= 0) return MINER_EINVAL;
  if (!aligned16(history) || !aligned16(packed) || !aligned16(user_mui) || !aligned16(user_proj) || !aligned16(mui_f32))
    return MINER_EALIGN;
  if (U == 0) return MINER_OK;
  UeParams prm{};
  prm.hist = history; prm.his_ids = his_ids; prm.n_news = n_news; prm.mask = his_mask; prm.bias = his_bias;
  prm.wp = packed; prm.mui_f32 = mui_f32; prm.user_mui = user_mui; prm.user_proj = user_proj;
  prm.U = U; prm.L = L; prm.d = d; prm.Dc = Dc; prm.K = K;
  if (dtype == MINER_DTYPE_BF16) return ue_dispatch<__bf16>(stream, prm);
  if (dtype == MINER_DTYPE_F16) return ue_dispatch<_Float16>(stream, prm);
  return ue_dispatch<float>(stream, prm);
}

size_t miner_rank_topk_workspace_bytes(int U, int topk) {
  if (U <= 0 || topk <= 0 || topk > kMaxTopk || num_cus() != 256) return 0;
  return rk_ws_bytes(U, topk);
}

int miner_rank_topk_split_recommended(int U) { return U > 0 && rk_split_wanted(U) ? 1 : 0; }

int miner_rank_topk(void* stream, int dtype, int score_type, const void* user_mui, const void* user_proj,
                    const void* news, int U, int N, int d, int K, int topk, float* top_scores, int32_t* top_ids) {
  RkParams prm = rk_params(score_type, user_mui, user_proj, news, U, N, d, K, topk, top_scores, top_ids);
  return rk_run(stream, dtype, prm, nullptr, 0);
}

int miner_rank_topk_ws(void* stream, int dtype, int score_type, const void* user_mui, const void* user_proj,
                       const void* news, int U, int N, int d, int K, int topk, float* top_scores, int32_t* top_ids,
                       void* workspace, size_t workspace_bytes) {
  RkParams prm = rk_params(score_type, user_mui, user_proj, news, U, N, d, K, topk, top_scores, top_ids);
  return rk_run(stream, dtype, prm, workspace, workspace_bytes);
}

int miner_rank_topk_filtered(void* stream, int dtype, int score_type, const void* user_mui, const void* user_proj,
                             const void* news, int U, int N, int d, int K, int topk, const int32_t* exclude_ids, int E,
                             const uint32_t* news_ok, float* top_scores, int32_t* top_ids, void* workspace,
                             size_t workspace_bytes) {
  RkParams prm = rk_params(score_type, user_mui, user_proj, news, U, N, d, K, topk, top_scores, top_ids);
  prm.excl = exclude_ids; prm.E = E; prm.ok = news_ok;
  return rk_run(stream, dtype, prm, workspace, workspace_bytes);
}

int miner_rank_topk_subset(void* stream, int dtype, int score_type, const void* user_mui, const void* user_proj,
                           const void* news, int U, int N, int d, int K, int topk, const int32_t* exclude_ids, int E,
                           const uint32_t* news_ok, const int32_t* news_ids, int M, float* top_scores, int32_t* top_ids,
                           void* workspace, size_t workspace_bytes) {
  RkParams prm = rk_params(score_type, user_mui, user_proj, news, U, N, d, K, topk, top_scores, top_ids);
  prm.excl = exclude_ids; prm.E = E; prm.ok = news_ok;
  // Here a NULL list with M < 0 is an error, for the wider entries it is the whole table: that pair
  // goes on with a list pointer that is never read, so that M < 0 answers at the list's check.
  static const int32_t no_list = 0;
  prm.ids = news_ids == nullptr && M < 0 ? &no_list : news_ids; prm.M = M;
  return rk_run(stream, dtype, prm, workspace, workspace_bytes);
}

int miner_rank_topk_biased(void* stream, int dtype, int score_type, const void* user_mui, const void* user_proj,
                           const void* news, int U, int N, int d, int K, int topk, const int32_t* exclude_ids, int E,
                           const uint32_t* news_ok, const int32_t* news_ids, int M, float* top_scores, int32_t* top_ids,
                           void* workspace, size_t workspace_bytes, const float* news_bias, int G,
                           const int32_t* user_group) {
  RkParams prm = rk_params(score_type, user_mui, user_proj, news, U, N, d, K, topk, top_scores, top_ids);
  prm.excl = exclude_ids; prm.E = E; prm.ok = news_ok;
  prm.ids = news_ids; prm.M = M;
  prm.bias = news_bias; prm.G = G; prm.grp = user_group;
  return rk_run(stream, dtype, prm, workspace, workspace_bytes);
}

int miner_rank_topk_capped(void* stream, int dtype, int score_type, const void* user_mui, const void* user_proj,
                           const void* news, int U, int N, int d, int K, int topk, const int32_t* exclude_ids, int E,
                           const uint32_t* news_ok, const int32_t* news_ids, int M, float* top_scores, int32_t* top_ids,
                           void* workspace, size_t workspace_bytes, const float* news_bias, int G,
                           const int32_t* user_group, const int32_t* news_cluster, int cap) {
  RkParams prm = rk_params(score_type, user_mui, user_proj, news, U, N, d, K, topk, top_scores, top_ids);
  prm.excl = exclude_ids; prm.E = E; prm.ok = news_ok;
  prm.ids = news_ids; prm.M = M;
  prm.bias = news_bias; prm.G = G; prm.grp = user_group;
  prm.clus = news_cluster; prm.cap = cap;
  return rk_run(stream, dtype, prm, workspace, workspace_bytes);
}

int miner_rank_topk_after(void* stream, int dtype, int score_type, const void* user_mui, const void* user_proj,
                          const void* news, int U, int N, int d, int K, int topk, const int32_t* exclude_ids, int E,
                          const uint32_t* news_ok, const int32_t* news_ids, int M, float* top_scores, int32_t* top_ids,
                          void* workspace, size_t workspace_bytes, const float* news_bias, int G,
                          const int32_t* user_group, const int32_t* news_cluster, int cap, const float* after_scores,
                          const int32_t* after_ids) {
  RkParams prm = rk_params(score_type, user_mui, user_proj, news, U, N, d, K, topk, top_scores, top_ids);
  prm.excl = exclude_ids; prm.E = E; prm.ok = news_ok;
  prm.ids = news_ids; prm.M = M;
  prm.bias = news_bias; prm.G = G; prm.grp = user_group;
  prm.clus = news_cluster; prm.cap = cap;
  prm.aft_s = after_scores; prm.aft_i = after_ids;
  return rk_run(stream, dtype, prm, workspace, workspace_bytes);
}

int miner_rank_topk_interest(void* stream, int dtype, int score_type, const void* user_mui, const void* user_proj,
                             const void* news, int U, int N, int d, int K, int topk, const int32_t* exclude_ids, int E,
                             const uint32_t* news_ok, const int32_t* news_ids, int M, float* top_scores, int32_t* top_ids,
                             void* workspace, size_t workspace_bytes, const float* news_bias, int G,
                             const int32_t* user_group, const int32_t* news_cluster, int cap, const float* after_scores,
                             const int32_t* after_ids, int interest_cap, int32_t* top_interest) {
  RkParams prm = rk_params(score_type, user_mui, user_proj, news, U, N, d, K, topk, top_scores, top_ids);
  prm.excl = exclude_ids; prm.E = E; prm.ok = news_ok;
  prm.ids = news_ids; prm.M = M;
  prm.bias = news_bias; prm.G = G; prm.grp = user_group;
  prm.clus = news_cluster; prm.cap = cap;
  prm.aft_s = after_scores; prm.aft_i = after_ids;
  prm.icap = interest_cap; prm.top_g = top_interest;
  return rk_run(stream, dtype, prm, workspace, workspace_bytes);
}

int miner_rank_topk_resume(void* stream, int dtype, int score_type, const void* user_mui, const void* user_proj,
                           const void* news, int U, int N, int d, int K, int topk, const int32_t* exclude_ids, int E,
                           const uint32_t* news_ok, const int32_t* news_ids, int M, float* top_scores, int32_t* top_ids,
                           void* workspace, size_t workspace_bytes, const float* news_bias, int G,
                           const int32_t* user_group, const int32_t* news_cluster, int cap, const float* after_scores,
                           const int32_t* after_ids, int interest_cap, int32_t* top_interest, const int32_t* used_groups,
                           const int32_t* used_counts, const int32_t* n_used, int Q) {
  RkParams prm = rk_params(score_type, user_mui, user_proj, news, U, N, d, K, topk, top_scores, top_ids);
  prm.excl = exclude_ids; prm.E = E; prm.ok = news_ok;
  prm.ids = news_ids; prm.M = M;
  prm.bias = news_bias; prm.G = G; prm.grp = user_group;
  prm.clus = news_cluster; prm.cap = cap;
  prm.aft_s = after_scores; prm.aft_i = after_ids;
  prm.icap = interest_cap; prm.top_g = top_interest;
  prm.use_g = used_groups; prm.use_c = used_counts; prm.use_n = n_used; prm.Q = Q;   // all NULL: no table, Q is not read
  return rk_run(stream, dtype, prm, workspace, workspace_bytes);
}

int miner_walk_advance(void* stream, const float* page_scores, const int32_t* page_ids, const int32_t* page_groups,
                       const int32_t* news_cluster, int n_cluster, const int32_t* in_groups, const int32_t* in_counts,
                       const int32_t* in_n_used, int Q_in, float* out_after_scores, int32_t* out_after_ids,
                       int32_t* out_groups, int32_t* out_counts, int32_t* out_n_used, uint8_t* overflow, int U, int k,
                       int Q) {
  if (U < 0 || k <= 0 || Q < 0 || Q_in < 0) return MINER_EINVAL;
  if (k > kMaxTopk || Q > kMaxWalk || Q_in > kMaxWalk) return MINER_ESHAPE;
  if (!page_scores || !page_ids || !in_n_used || !out_after_scores || !out_after_ids || !out_n_used || !overflow)
    return MINER_EINVAL;
  if ((Q_in > 0 && (!in_groups || !in_counts)) || (Q > 0 && (!out_groups || !out_counts))) return MINER_EINVAL;
  if (page_groups == nullptr && (news_cluster == nullptr || n_cluster <= 0)) return MINER_EINVAL;
  if (!aligned4(page_scores) || !aligned4(page_ids) || !aligned4(page_groups) || !aligned4(news_cluster) ||
      !aligned4(in_groups) || !aligned4(in_counts) || !aligned4(in_n_used) || !aligned4(out_after_scores) ||
      !aligned4(out_after_ids) || !aligned4(out_groups) || !aligned4(out_counts) || !aligned4(out_n_used))
    return MINER_EALIGN;
  if (U == 0) return MINER_OK;
  hipLaunchKernelGGL(walk_advance, dim3((U + kMergeUsers - 1) / kMergeUsers), dim3(64 * kMergeUsers), 0,
                     static_cast<hipStream_t>(stream), page_scores, page_ids, page_groups, news_cluster, n_cluster, in_groups,
                     in_counts, in_n_used, Q_in, out_after_scores, out_after_ids, out_groups, out_counts, out_n_used, overflow,
                     U, k, Q);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MINER_OK : (int)e;
}

int miner_topk_merge(void* stream, const float* a_scores, const int32_t* a_ids, int ka, const float* b_scores,
                     const int32_t* b_ids, int kb, int U, int topk, const uint32_t* news_ok, int N, float* out_scores,
                     int32_t* out_ids) {
  return miner_topk_merge_capped(stream, a_scores, a_ids, ka, b_scores, b_ids, kb, U, topk, news_ok, N, out_scores, out_ids,
                                 nullptr, 0, 0);
}

int miner_topk_merge_capped(void* stream, const float* a_scores, const int32_t* a_ids, int ka, const float* b_scores,
                            const int32_t* b_ids, int kb, int U, int topk, const uint32_t* news_ok, int N,
                            float* out_scores, int32_t* out_ids, const int32_t* news_cluster, int n_cluster, int cap) {
  const int ck = merge_check(a_scores, a_ids, ka, b_scores, b_ids, kb, U, topk, news_ok, N, out_scores, out_ids);
  if (ck != MINER_OK) return ck;
  const int cc = cap_check(news_cluster, cap);
  if (cc != MINER_OK) return cc;
  if (news_cluster != nullptr && n_cluster <= 0) return MINER_EINVAL;
  if (!aligned4(news_cluster)) return MINER_EALIGN;
  if (U == 0) return MINER_OK;
  // (the capped instantiation only with a table: the plain merge launches the kernel it did)
  return merge_launch(news_cluster != nullptr ? topk_merge<1> : topk_merge<0>, stream, a_scores, a_ids, ka, b_scores, b_ids,
                      kb, U, topk, news_ok, N, out_scores, out_ids, news_cluster, n_cluster, cap, nullptr, nullptr, nullptr);
}

int miner_topk_merge_grouped(void* stream, const float* a_scores, const int32_t* a_ids, int ka, const float* b_scores,
                             const int32_t* b_ids, int kb, int U, int topk, const uint32_t* news_ok, int N,
                             float* out_scores, int32_t* out_ids, const int32_t* a_groups, const int32_t* b_groups,
                             int32_t* out_groups, int cap) {
  const int ck = merge_check(a_scores, a_ids, ka, b_scores, b_ids, kb, U, topk, news_ok, N, out_scores, out_ids);
  if (ck != MINER_OK) return ck;
  if (cap < 0) return MINER_EINVAL;
  if (cap > kMaxTopk) return MINER_ESHAPE;
  if ((ka > 0 && !a_groups) || (kb > 0 && !b_groups) || !out_groups) return MINER_EINVAL;
  if (!aligned4(a_groups) || !aligned4(b_groups) || !aligned4(out_groups)) return MINER_EALIGN;
  if (U == 0) return MINER_OK;
  return merge_launch(topk_merge<2>, stream, a_scores, a_ids, ka, b_scores, b_ids, kb, U, topk, news_ok, N, out_scores,
                      out_ids, nullptr, 0, cap, a_groups, b_groups, out_groups);
}

}  // extern "C"
