// Host-side argument validation of miner_rank_topk_capped and miner_topk_merge_capped
// (include/miner_corpus.h), built like abi_errors_bias.cpp (host code under AddressSanitizer,
// miner_amd/build.py --asan) and run on a CPU-only machine by tests/test_corpus_cap_host.py: the
// cluster table's checks return their documented MINER_E* codes after the base call's own checks and
// before any device work, the accepted argument sets return MINER_OK with U = 0, so nothing launches,
// and ASan must report nothing. The pointers are host addresses that a correct validation never
// dereferences: `buf` is 16-byte aligned, `mis` is 4-byte but not 16-byte aligned, the `odd` ones are
// not 4-byte aligned.
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
  const float* fodd = (const float*)(g_buf + 2);
  float* fo = (float*)(g_buf + 1024);
  int32_t* io = (int32_t*)(g_buf + 2048);
  void* st = nullptr;
  const int F16 = MINER_DTYPE_F16, W = MINER_SCORE_WEIGHTED;

  if (miner_abi_version() != MINER_ABI_VERSION || MINER_ABI_VERSION != 6) { fprintf(stderr, "FAIL abi version\n"); ++g_fail; }

  // ---- miner_rank_topk_capped: the table's checks, with users (no launch) and without ----
  for (int U = 0; U <= 4; U += 4) {
    EXPECT(miner_rank_topk_capped(st, F16, W, buf, buf, buf, U, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, fb, 1, nullptr, ib, 0), MINER_EINVAL);
    EXPECT(miner_rank_topk_capped(st, F16, W, buf, buf, buf, U, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, nullptr, 0, nullptr, ib, -3), MINER_EINVAL);
    EXPECT(miner_rank_topk_capped(st, F16, W, buf, buf, buf, U, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, nullptr, 0, nullptr, ib, 257), MINER_ESHAPE);
    EXPECT(miner_rank_topk_capped(st, F16, W, buf, buf, buf, U, 1000, 768, 64, 100, ib, 3, wb, ib, 5, fo, io, nullptr, 0, nullptr, 0, nullptr, iodd, 2), MINER_EALIGN);
    EXPECT(miner_rank_topk_capped(st, F16, W, buf, buf, buf, U, 1000, 768, 64, 100, ib, 3, wb, ib, 5, fo, io, nullptr, 0, nullptr, 0, nullptr, iodd, 0), MINER_EINVAL);    // cap before the alignment
    EXPECT(miner_rank_topk_capped(st, F16, W, buf, buf, buf, U, 1000, 768, 64, 100, ib, 3, wb, ib, 5, fo, io, nullptr, 0, nullptr, 0, nullptr, iodd, 999), MINER_ESHAPE);
  }
  // the older checks first, each with bad caps as well
  EXPECT(miner_rank_topk_capped(st, 9, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, fb, 1, nullptr, iodd, 0), MINER_EINVAL);
  EXPECT(miner_rank_topk_capped(st, F16, W, buf, buf, buf, 4, 1000, 100, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, fb, 1, nullptr, iodd, 0), MINER_ESHAPE);
  EXPECT(miner_rank_topk_capped(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 257, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, fb, 1, nullptr, iodd, 0), MINER_ESHAPE);
  EXPECT(miner_rank_topk_capped(st, F16, W, mis, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, fb, 1, nullptr, iodd, 0), MINER_EALIGN);
  EXPECT(miner_rank_topk_capped(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 257, wb, nullptr, -1, fo, io, nullptr, 0, fb, 1, nullptr, iodd, 0), MINER_ESHAPE);
  EXPECT(miner_rank_topk_capped(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, iodd, 5, fo, io, nullptr, 0, fb, 1, nullptr, ib, 0), MINER_EALIGN);          // the id list first
  EXPECT(miner_rank_topk_capped(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, fb, 0, nullptr, ib, 0), MINER_EINVAL);       // the prior first
  EXPECT(miner_rank_topk_capped(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, fodd, 1, nullptr, ib, 257), MINER_EALIGN);   // the prior's alignment first
  // accepted argument sets: U == 0 returns after the validation
  EXPECT(miner_rank_topk_capped(st, F16, W, buf, buf, buf, 0, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, fb, 3, ib, ib, 1), MINER_OK);
  EXPECT(miner_rank_topk_capped(st, F16, W, buf, buf, buf, 0, 1000, 768, 64, 100, nullptr, 0, nullptr, ib, 5, fo, io, nullptr, 0, nullptr, 0, nullptr, imis, 256), MINER_OK);
  EXPECT(miner_rank_topk_capped(st, F16, W, buf, buf, buf, 0, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, buf, 64, nullptr, 0, nullptr, ib, 2), MINER_OK);       // a workspace is accepted
  EXPECT(miner_rank_topk_capped(st, F16, W, buf, buf, buf, 0, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, fb, 1, nullptr, nullptr, 0), MINER_OK);     // no table: the biased call
  EXPECT(miner_rank_topk_capped(st, F16, W, buf, buf, buf, 0, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, nullptr, 0, nullptr, nullptr, -5), MINER_OK);  // cap is read only with a table
  EXPECT(miner_rank_topk_capped(st, F16, W, buf, buf, buf, 0, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, nullptr, 0, nullptr, nullptr, 9999), MINER_OK);

  // ---- miner_topk_merge_capped ----
  for (int U = 0; U <= 4; U += 4) {
    EXPECT(miner_topk_merge_capped(st, fb, ib, 100, fb, ib, 100, U, 100, wb, 1000, fo, io, ib, 1000, 0), MINER_EINVAL);
    EXPECT(miner_topk_merge_capped(st, fb, ib, 100, fb, ib, 100, U, 100, wb, 1000, fo, io, ib, 1000, -1), MINER_EINVAL);
    EXPECT(miner_topk_merge_capped(st, fb, ib, 100, fb, ib, 100, U, 100, wb, 1000, fo, io, ib, 1000, 257), MINER_ESHAPE);
    EXPECT(miner_topk_merge_capped(st, fb, ib, 100, fb, ib, 100, U, 100, wb, 1000, fo, io, ib, 0, 2), MINER_EINVAL);
    EXPECT(miner_topk_merge_capped(st, fb, ib, 100, fb, ib, 100, U, 100, nullptr, 0, fo, io, ib, -7, 2), MINER_EINVAL);
    EXPECT(miner_topk_merge_capped(st, fb, ib, 100, fb, ib, 100, U, 100, nullptr, 0, fo, io, iodd, 1000, 2), MINER_EALIGN);
    EXPECT(miner_topk_merge_capped(st, fb, ib, 100, fb, ib, 100, U, 100, nullptr, 0, fo, io, iodd, 0, 2), MINER_EINVAL);       // n_cluster before the alignment
    EXPECT(miner_topk_merge_capped(st, fb, ib, 100, fb, ib, 100, U, 100, nullptr, 0, fo, io, iodd, 0, 257), MINER_ESHAPE);     // cap before n_cluster
  }
  // the base call's checks first, each with bad caps as well
  EXPECT(miner_topk_merge_capped(st, fb, ib, -1, fb, ib, 100, 4, 100, wb, 1000, fo, io, iodd, 0, 0), MINER_EINVAL);
  EXPECT(miner_topk_merge_capped(st, fb, ib, 257, fb, ib, 100, 4, 100, wb, 1000, fo, io, iodd, 0, 0), MINER_ESHAPE);
  EXPECT(miner_topk_merge_capped(st, fb, ib, 100, fb, ib, 100, 4, 0, wb, 1000, fo, io, iodd, 0, 0), MINER_EINVAL);
  EXPECT(miner_topk_merge_capped(st, fb, nullptr, 100, fb, ib, 100, 4, 100, wb, 1000, fo, io, iodd, 0, 0), MINER_EINVAL);
  EXPECT(miner_topk_merge_capped(st, fb, ib, 100, fb, ib, 100, 4, 100, wb, 0, fo, io, iodd, 0, 0), MINER_EINVAL);              // a bitmap with N <= 0
  EXPECT(miner_topk_merge_capped(st, fodd, ib, 100, fb, ib, 100, 4, 100, wb, 1000, fo, io, ib, 1000, 257), MINER_EALIGN);
  // accepted argument sets
  EXPECT(miner_topk_merge_capped(st, fb, ib, 100, fb, ib, 100, 0, 100, wb, 1000, fo, io, ib, 1000, 1), MINER_OK);
  EXPECT(miner_topk_merge_capped(st, nullptr, nullptr, 0, fb, ib, 256, 0, 256, nullptr, 0, fo, io, imis, 1, 256), MINER_OK);
  EXPECT(miner_topk_merge_capped(st, fb, ib, 100, fb, ib, 100, 0, 100, wb, 1000, fo, io, nullptr, 0, 0), MINER_OK);            // no table: miner_topk_merge
  EXPECT(miner_topk_merge_capped(st, fb, ib, 100, fb, ib, 100, 0, 100, wb, 1000, fo, io, nullptr, -4, 9999), MINER_OK);        // read only with a table

  printf("abi_errors_cap: %d calls, %d failures\n", g_calls, g_fail);
  return g_fail ? 1 : 0;
}
