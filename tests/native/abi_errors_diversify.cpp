// Host-side argument validation of miner_topk_diversify (include/miner_diversify.h), built like
// abi_errors_cap.cpp (host code under AddressSanitizer, miner_amd/build.py --asan) and run on a
// CPU-only machine by tests/test_corpus_diversify_host.py: every argument error returns its
// documented MINER_E* code in the documented order and before any device work, the accepted
// argument sets return MINER_OK with U = 0, so nothing launches, and ASan must report nothing. The
// pointers are host addresses that a correct validation never dereferences: `buf` is 16-byte
// aligned, `mis` is 4-byte but not 16-byte aligned, the `odd` ones are not 4-byte aligned.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "miner_diversify.h"

alignas(16) static unsigned char g_buf[4096];

static int g_fail = 0, g_calls = 0;
static void expect(const char* what, int rc, int want) {
  ++g_calls;
  if (rc != want) {
    fprintf(stderr, "FAIL %s: rc %d, want %d\n", what, rc, want);
    ++g_fail;
  }
}
#define EXPECT(call, want) expect(#call, (call), (want))

int main() {
  void* buf = g_buf;
  void* mis = g_buf + 4;
  const float* fs = (const float*)(g_buf + 256);
  const float* fodd = (const float*)(g_buf + 258);
  const int32_t* ii = (const int32_t*)(g_buf + 512);
  const int32_t* iodd = (const int32_t*)(g_buf + 514);
  float* os = (float*)(g_buf + 1024);
  float* osodd = (float*)(g_buf + 1026);
  int32_t* oi = (int32_t*)(g_buf + 2048);
  int32_t* oiodd = (int32_t*)(g_buf + 2050);
  int32_t* op = (int32_t*)(g_buf + 3072);
  int32_t* opodd = (int32_t*)(g_buf + 3074);
  float* oo = (float*)(g_buf + 3584);
  float* ooodd = (float*)(g_buf + 3586);
  void* st = nullptr;
  const int F16 = MINER_DTYPE_F16, BF16 = MINER_DTYPE_BF16, F32 = MINER_DTYPE_F32;
  const int MM = MINER_DIVERSIFY_REL_MINMAX, SC = MINER_DIVERSIFY_REL_SCORE;

  if (miner_abi_version() != MINER_ABI_VERSION || MINER_ABI_VERSION != 6) { fprintf(stderr, "FAIL abi version\n"); ++g_fail; }

  for (int U = 0; U <= 4; U += 4) {   // with users too: still no launch
    // 1. dtype, relevance
    EXPECT(miner_topk_diversify(st, 9, buf, 1000, 768, fs, ii, U, 256, 100, 0.7f, MM, os, oi, op, oo), MINER_EINVAL);
    EXPECT(miner_topk_diversify(st, MINER_DTYPE_F32_MFMA, buf, 1000, 768, fs, ii, U, 256, 100, 0.7f, MM, os, oi, op, oo), MINER_EINVAL);
    EXPECT(miner_topk_diversify(st, -1, buf, 1000, 768, fs, ii, U, 256, 100, 0.7f, MM, os, oi, op, oo), MINER_EINVAL);
    EXPECT(miner_topk_diversify(st, F16, buf, 1000, 768, fs, ii, U, 256, 100, 0.7f, 2, os, oi, op, oo), MINER_EINVAL);
    EXPECT(miner_topk_diversify(st, F16, buf, 1000, 768, fs, ii, U, 256, 100, 0.7f, -1, os, oi, op, oo), MINER_EINVAL);
    // 2. sizes
    EXPECT(miner_topk_diversify(st, F16, buf, 0, 768, fs, ii, U, 256, 100, 0.7f, MM, os, oi, op, oo), MINER_EINVAL);
    EXPECT(miner_topk_diversify(st, F16, buf, 1000, 768, fs, ii, U, 0, 100, 0.7f, MM, os, oi, op, oo), MINER_EINVAL);
    EXPECT(miner_topk_diversify(st, F16, buf, 1000, 768, fs, ii, U, 256, 0, 0.7f, MM, os, oi, op, oo), MINER_EINVAL);
    EXPECT(miner_topk_diversify(st, F16, buf, 1000, 768, fs, ii, U, -3, -3, 0.7f, MM, os, oi, op, oo), MINER_EINVAL);
    // 3. required pointers
    EXPECT(miner_topk_diversify(st, F16, nullptr, 1000, 768, fs, ii, U, 256, 100, 0.7f, MM, os, oi, op, oo), MINER_EINVAL);
    EXPECT(miner_topk_diversify(st, F16, buf, 1000, 768, nullptr, ii, U, 256, 100, 0.7f, MM, os, oi, op, oo), MINER_EINVAL);
    EXPECT(miner_topk_diversify(st, F16, buf, 1000, 768, fs, nullptr, U, 256, 100, 0.7f, MM, os, oi, op, oo), MINER_EINVAL);
    EXPECT(miner_topk_diversify(st, F16, buf, 1000, 768, fs, ii, U, 256, 100, 0.7f, MM, nullptr, oi, op, oo), MINER_EINVAL);
    EXPECT(miner_topk_diversify(st, F16, buf, 1000, 768, fs, ii, U, 256, 100, 0.7f, MM, os, nullptr, op, oo), MINER_EINVAL);
    EXPECT(miner_topk_diversify(st, F16, buf, 1000, 768, fs, ii, U, 256, 100, 0.7f, MM, os, oi, nullptr, oo), MINER_EINVAL);
    // 4. lambda
    EXPECT(miner_topk_diversify(st, F16, buf, 1000, 768, fs, ii, U, 256, 100, -0.01f, MM, os, oi, op, oo), MINER_EINVAL);
    EXPECT(miner_topk_diversify(st, F16, buf, 1000, 768, fs, ii, U, 256, 100, 1.5f, MM, os, oi, op, oo), MINER_EINVAL);
    EXPECT(miner_topk_diversify(st, F16, buf, 1000, 768, fs, ii, U, 256, 100, NAN, MM, os, oi, op, oo), MINER_EINVAL);
    EXPECT(miner_topk_diversify(st, F16, buf, 1000, 768, fs, ii, U, 256, 100, INFINITY, MM, os, oi, op, oo), MINER_EINVAL);
    // 5. shapes
    EXPECT(miner_topk_diversify(st, F16, buf, 1000, 768, fs, ii, U, 257, 100, 0.7f, MM, os, oi, op, oo), MINER_ESHAPE);
    EXPECT(miner_topk_diversify(st, F16, buf, 1000, 768, fs, ii, U, 100, 101, 0.7f, MM, os, oi, op, oo), MINER_ESHAPE);
    EXPECT(miner_topk_diversify(st, F16, buf, 1000, 0, fs, ii, U, 256, 100, 0.7f, MM, os, oi, op, oo), MINER_ESHAPE);
    EXPECT(miner_topk_diversify(st, F16, buf, 1000, 96, fs, ii, U, 256, 100, 0.7f, MM, os, oi, op, oo), MINER_ESHAPE);
    EXPECT(miner_topk_diversify(st, BF16, buf, 1000, 32, fs, ii, U, 256, 100, 0.7f, MM, os, oi, op, oo), MINER_ESHAPE);
    EXPECT(miner_topk_diversify(st, F32, buf, 1000, 48, fs, ii, U, 256, 100, 0.7f, MM, os, oi, op, oo), MINER_ESHAPE);
    EXPECT(miner_topk_diversify(st, F16, buf, 1000, 1088, fs, ii, U, 256, 100, 0.7f, MM, os, oi, op, oo), MINER_ESHAPE);
    // 6. alignment
    EXPECT(miner_topk_diversify(st, F16, mis, 1000, 768, fs, ii, U, 256, 100, 0.7f, MM, os, oi, op, oo), MINER_EALIGN);
    EXPECT(miner_topk_diversify(st, F16, buf, 1000, 768, fodd, ii, U, 256, 100, 0.7f, MM, os, oi, op, oo), MINER_EALIGN);
    EXPECT(miner_topk_diversify(st, F16, buf, 1000, 768, fs, iodd, U, 256, 100, 0.7f, MM, os, oi, op, oo), MINER_EALIGN);
    EXPECT(miner_topk_diversify(st, F16, buf, 1000, 768, fs, ii, U, 256, 100, 0.7f, MM, osodd, oi, op, oo), MINER_EALIGN);
    EXPECT(miner_topk_diversify(st, F16, buf, 1000, 768, fs, ii, U, 256, 100, 0.7f, MM, os, oiodd, op, oo), MINER_EALIGN);
    EXPECT(miner_topk_diversify(st, F16, buf, 1000, 768, fs, ii, U, 256, 100, 0.7f, MM, os, oi, opodd, oo), MINER_EALIGN);
    EXPECT(miner_topk_diversify(st, F16, buf, 1000, 768, fs, ii, U, 256, 100, 0.7f, MM, os, oi, op, ooodd), MINER_EALIGN);
    // the order: each class with every later class wrong as well
    EXPECT(miner_topk_diversify(st, 9, nullptr, 0, 100, fodd, iodd, -1, 300, 400, 2.f, MM, os, oi, op, oo), MINER_EINVAL);
    EXPECT(miner_topk_diversify(st, F16, mis, 1000, 100, fodd, ii, U, 300, 400, 2.f, MM, os, oi, op, oo), MINER_EINVAL);   // lambda before shape
    EXPECT(miner_topk_diversify(st, F16, mis, 1000, 100, fodd, ii, U, 300, 400, 0.5f, MM, os, oi, op, oo), MINER_ESHAPE);  // shape before alignment
    EXPECT(miner_topk_diversify(st, F16, mis, 1000, 768, fs, ii, U, 257, 100, 0.5f, MM, os, oi, op, oo), MINER_ESHAPE);
    EXPECT(miner_topk_diversify(st, F16, mis, 1000, 768, nullptr, ii, U, 257, 100, 7.f, MM, os, oi, op, oo), MINER_EINVAL);  // pointer before lambda
  }
  EXPECT(miner_topk_diversify(st, F16, buf, 1000, 768, fs, ii, -1, 256, 100, 0.7f, MM, os, oi, op, oo), MINER_EINVAL);
  EXPECT(miner_topk_diversify(st, F16, mis, 1000, 768, fs, ii, 0, 256, 100, 0.7f, MM, os, oi, op, oo), MINER_EALIGN);      // before the U == 0 return
  // accepted argument sets: U == 0 returns after the validation
  EXPECT(miner_topk_diversify(st, F16, buf, 1000, 768, fs, ii, 0, 256, 100, 0.7f, MM, os, oi, op, oo), MINER_OK);
  EXPECT(miner_topk_diversify(st, BF16, buf, 1, 64, fs, ii, 0, 1, 1, 0.f, SC, os, oi, op, nullptr), MINER_OK);            // out_obj is optional
  EXPECT(miner_topk_diversify(st, F32, buf, 1000, 32, fs, ii, 0, 256, 256, 1.f, MM, os, oi, op, oo), MINER_OK);
  EXPECT(miner_topk_diversify(st, F32, buf, 2147483647, 1024, fs, ii, 0, 100, 10, 0.3f, SC, os, oi, op, oo), MINER_OK);

  printf("abi_errors_diversify: %d calls, %d failures\n", g_calls, g_fail);
  return g_fail ? 1 : 0;
}
