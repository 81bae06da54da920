// Host-side argument validation of miner_rank_topk_after (include/miner_corpus.h), built like
// abi_errors_cap.cpp (host code under AddressSanitizer, miner_amd/build.py --asan) and run on a
// CPU-only machine by tests/test_corpus_after_host.py: the cursor's checks return their documented
// MINER_E* codes after the capped call's own checks and before any device work, the accepted argument
// sets return MINER_OK with U = 0, so nothing launches, and ASan must report nothing. The pointers are
// host addresses that a correct validation never dereferences: `buf` is 16-byte aligned, `mis` is
// 4-byte but not 16-byte aligned, the `odd` ones are not 4-byte aligned.
#include <stdint.h>
#include <stdio.h>

#include "miner_corpus.h"

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
  const int32_t* ib = (const int32_t*)g_buf;
  const int32_t* imis = (const int32_t*)(g_buf + 4);
  const int32_t* iodd = (const int32_t*)(g_buf + 2);
  const uint32_t* wb = (const uint32_t*)g_buf;
  const float* fb = (const float*)g_buf;
  const float* fmis = (const float*)(g_buf + 4);
  const float* fodd = (const float*)(g_buf + 2);
  float* fo = (float*)(g_buf + 1024);
  int32_t* io = (int32_t*)(g_buf + 2048);
  void* st = nullptr;
  const int F16 = MINER_DTYPE_F16, W = MINER_SCORE_WEIGHTED;

  if (miner_abi_version() != MINER_ABI_VERSION || MINER_ABI_VERSION != 6) { fprintf(stderr, "FAIL abi version\n"); ++g_fail; }

  // ---- the cursor's checks, with users (no launch) and without ----
  for (int U = 0; U <= 4; U += 4) {
    // one word without the other
    EXPECT(miner_rank_topk_after(st, F16, W, buf, buf, buf, U, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, fb, nullptr), MINER_EINVAL);
    EXPECT(miner_rank_topk_after(st, F16, W, buf, buf, buf, U, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, nullptr, ib), MINER_EINVAL);
    EXPECT(miner_rank_topk_after(st, F16, W, buf, buf, buf, U, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, fodd, nullptr), MINER_EINVAL);   // the pair before the alignment
    // a cursor together with a cluster table
    EXPECT(miner_rank_topk_after(st, F16, W, buf, buf, buf, U, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, nullptr, 0, nullptr, ib, 2, fb, ib), MINER_EINVAL);
    EXPECT(miner_rank_topk_after(st, F16, W, buf, buf, buf, U, 1000, 768, 64, 100, ib, 3, wb, ib, 5, fo, io, nullptr, 0, fb, 1, nullptr, ib, 2, fodd, iodd), MINER_EINVAL);          // ... before the alignment
    // alignment
    EXPECT(miner_rank_topk_after(st, F16, W, buf, buf, buf, U, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, fodd, ib), MINER_EALIGN);
    EXPECT(miner_rank_topk_after(st, F16, W, buf, buf, buf, U, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, fb, iodd), MINER_EALIGN);
    EXPECT(miner_rank_topk_after(st, F16, W, buf, buf, buf, U, 1000, 768, 64, 100, nullptr, 0, nullptr, ib, 5, fo, io, nullptr, 0, fb, 2, ib, nullptr, 0, fodd, iodd), MINER_EALIGN);
  }
  // the older checks first, each with a bad cursor as well
  EXPECT(miner_rank_topk_after(st, 9, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, fb, 1, nullptr, nullptr, 0, fodd, nullptr), MINER_EINVAL);
  EXPECT(miner_rank_topk_after(st, F16, W, buf, buf, buf, 4, 1000, 100, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, fb, 1, nullptr, nullptr, 0, fodd, nullptr), MINER_ESHAPE);
  EXPECT(miner_rank_topk_after(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 257, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, fb, 1, nullptr, nullptr, 0, fodd, nullptr), MINER_ESHAPE);
  EXPECT(miner_rank_topk_after(st, F16, W, mis, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, fb, 1, nullptr, nullptr, 0, fb, nullptr), MINER_EALIGN);
  EXPECT(miner_rank_topk_after(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 257, wb, nullptr, -1, fo, io, nullptr, 0, fb, 1, nullptr, nullptr, 0, fb, nullptr), MINER_ESHAPE);
  EXPECT(miner_rank_topk_after(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, iodd, 5, fo, io, nullptr, 0, fb, 1, nullptr, nullptr, 0, fb, nullptr), MINER_EALIGN);      // the id list first
  EXPECT(miner_rank_topk_after(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, fodd, 1, nullptr, nullptr, 0, fb, nullptr), MINER_EALIGN);  // the prior first
  EXPECT(miner_rank_topk_after(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, nullptr, 0, nullptr, ib, 257, fb, nullptr), MINER_ESHAPE);  // the caps first
  EXPECT(miner_rank_topk_after(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, nullptr, 0, nullptr, iodd, 2, fb, nullptr), MINER_EALIGN);  // ... and their alignment
  // accepted argument sets: U == 0 returns after the validation
  EXPECT(miner_rank_topk_after(st, F16, W, buf, buf, buf, 0, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, fb, ib), MINER_OK);
  EXPECT(miner_rank_topk_after(st, F16, W, buf, buf, buf, 0, 1000, 768, 64, 100, nullptr, 0, nullptr, nullptr, -1, fo, io, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, fmis, imis), MINER_OK);  // 4-byte aligned, no filter
  EXPECT(miner_rank_topk_after(st, F16, W, buf, buf, buf, 0, 1000, 768, 64, 100, ib, 3, wb, ib, 5, fo, io, buf, 64, fb, 3, ib, nullptr, 0, fb, ib), MINER_OK);                      // subset, prior, workspace
  EXPECT(miner_rank_topk_after(st, F16, W, buf, buf, buf, 0, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, nullptr, 0, nullptr, nullptr, -5, fb, ib), MINER_OK);  // cap is read only with a table
  // no cursor: the capped call
  EXPECT(miner_rank_topk_after(st, F16, W, buf, buf, buf, 0, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, fb, 1, nullptr, ib, 2, nullptr, nullptr), MINER_OK);
  EXPECT(miner_rank_topk_after(st, F16, W, buf, buf, buf, 0, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr), MINER_OK);
  EXPECT(miner_rank_topk_after(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, nullptr, 0, nullptr, ib, 0, nullptr, nullptr), MINER_EINVAL);

  printf("abi_errors_after: %d calls, %d failures\n", g_calls, g_fail);
  return g_fail ? 1 : 0;
}
