// Host-side argument validation of miner_rank_topk_subset and miner_topk_merge (include/miner_corpus.h),
// built like abi_errors.cpp (host code under AddressSanitizer, miner_amd/build.py --asan) and run on
// a CPU-only machine by tests/test_corpus_subset_host.py: every error path of the two entry points
// returns its documented MINER_E* code before any device work, the accepted argument sets return
// MINER_OK with U = 0 (nothing launches), and ASan must report nothing. The pointers are host
// addresses that a correct validation never dereferences: `buf` is 16-byte aligned, `mis` is 4-byte
// but not 16-byte aligned, `odd` is not 4-byte aligned.
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
  const int32_t* iodd = (const int32_t*)(g_buf + 2);
  const uint32_t* wb = (const uint32_t*)g_buf;
  const uint32_t* wodd = (const uint32_t*)(g_buf + 6);
  const float* fb = (const float*)g_buf;
  const float* fodd = (const float*)(g_buf + 2);
  float* fo = (float*)(g_buf + 1024);
  float* foodd = (float*)(g_buf + 1026);
  int32_t* io = (int32_t*)(g_buf + 2048);
  int32_t* ioodd = (int32_t*)(g_buf + 2050);
  void* st = nullptr;
  const int F16 = MINER_DTYPE_F16, W = MINER_SCORE_WEIGHTED;

  if (miner_abi_version() != MINER_ABI_VERSION) { fprintf(stderr, "FAIL abi version\n"); ++g_fail; }

  // ---- miner_rank_topk_subset: the id list's own checks ----
  EXPECT(miner_rank_topk_subset(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 10, ib, 4, wb, ib, -1, fo, io, nullptr, 0), MINER_EINVAL);
  EXPECT(miner_rank_topk_subset(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 10, ib, 4, wb, nullptr, 5, fo, io, nullptr, 0), MINER_EINVAL);
  EXPECT(miner_rank_topk_subset(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 10, ib, 4, wb, iodd, 5, fo, io, nullptr, 0), MINER_EALIGN);
  EXPECT(miner_rank_topk_subset(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 10, ib, 4, wb, iodd, 0, fo, io, nullptr, 0), MINER_EALIGN);
  EXPECT(miner_rank_topk_subset(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 10, nullptr, 0, nullptr, ib, -2147483647 - 1, fo, io, nullptr, 0), MINER_EINVAL);
  EXPECT(miner_rank_topk_subset(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 10, ib, 4, wb, ib, 0, fo, io, mis, 1 << 20), MINER_EALIGN);
  // ---- the table forms' checks first, with their codes (each with a bad id list as well) ----
  EXPECT(miner_rank_topk_subset(st, 9, W, buf, buf, buf, 4, 1000, 768, 64, 10, ib, 4, wb, nullptr, -1, fo, io, nullptr, 0), MINER_EINVAL);
  EXPECT(miner_rank_topk_subset(st, F16, W, buf, buf, buf, 4, 1000, 100, 64, 10, ib, 4, wb, iodd, 5, fo, io, nullptr, 0), MINER_ESHAPE);
  EXPECT(miner_rank_topk_subset(st, F16, W, buf, buf, buf, 4, 1000, 768, 65, 10, ib, 4, wb, iodd, 5, fo, io, nullptr, 0), MINER_ESHAPE);
  EXPECT(miner_rank_topk_subset(st, F16, 7, buf, buf, buf, 4, 1000, 768, 64, 10, ib, 4, wb, iodd, 5, fo, io, nullptr, 0), MINER_EINVAL);
  EXPECT(miner_rank_topk_subset(st, F16, W, buf, buf, buf, -1, 1000, 768, 64, 10, ib, 4, wb, iodd, 5, fo, io, nullptr, 0), MINER_EINVAL);
  EXPECT(miner_rank_topk_subset(st, F16, W, buf, buf, buf, 4, 0, 768, 64, 10, ib, 4, wb, iodd, 5, fo, io, nullptr, 0), MINER_EINVAL);
  EXPECT(miner_rank_topk_subset(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 0, ib, 4, wb, iodd, 5, fo, io, nullptr, 0), MINER_EINVAL);
  EXPECT(miner_rank_topk_subset(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 257, ib, 4, wb, iodd, 5, fo, io, nullptr, 0), MINER_ESHAPE);
  EXPECT(miner_rank_topk_subset(st, F16, W, nullptr, buf, buf, 4, 1000, 768, 64, 10, ib, 4, wb, iodd, 5, fo, io, nullptr, 0), MINER_EINVAL);
  EXPECT(miner_rank_topk_subset(st, F16, W, buf, nullptr, buf, 4, 1000, 768, 64, 10, ib, 4, wb, iodd, 5, fo, io, nullptr, 0), MINER_EINVAL);
  EXPECT(miner_rank_topk_subset(st, F16, W, buf, buf, nullptr, 4, 1000, 768, 64, 10, ib, 4, wb, iodd, 5, fo, io, nullptr, 0), MINER_EINVAL);
  EXPECT(miner_rank_topk_subset(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 10, ib, 4, wb, iodd, 5, nullptr, io, nullptr, 0), MINER_EINVAL);
  EXPECT(miner_rank_topk_subset(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 10, ib, 4, wb, iodd, 5, fo, nullptr, nullptr, 0), MINER_EINVAL);
  EXPECT(miner_rank_topk_subset(st, F16, W, mis, buf, buf, 4, 1000, 768, 64, 10, ib, 4, wb, nullptr, 5, fo, io, nullptr, 0), MINER_EALIGN);
  EXPECT(miner_rank_topk_subset(st, F16, W, buf, mis, buf, 4, 1000, 768, 64, 10, ib, 4, wb, nullptr, 5, fo, io, nullptr, 0), MINER_EALIGN);
  EXPECT(miner_rank_topk_subset(st, F16, W, buf, buf, mis, 4, 1000, 768, 64, 10, ib, 4, wb, nullptr, 5, fo, io, nullptr, 0), MINER_EALIGN);
  EXPECT(miner_rank_topk_subset(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 10, ib, -1, wb, iodd, 5, fo, io, nullptr, 0), MINER_EINVAL);
  EXPECT(miner_rank_topk_subset(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 10, nullptr, 4, wb, iodd, 5, fo, io, nullptr, 0), MINER_EINVAL);
  EXPECT(miner_rank_topk_subset(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 10, ib, 257, wb, iodd, 5, fo, io, nullptr, 0), MINER_ESHAPE);
  EXPECT(miner_rank_topk_subset(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 10, iodd, 4, wb, nullptr, 5, fo, io, nullptr, 0), MINER_EALIGN);
  EXPECT(miner_rank_topk_subset(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 10, ib, 4, wodd, nullptr, 5, fo, io, nullptr, 0), MINER_EALIGN);
  // ---- accepted argument sets: U == 0 returns after the validation ----
  EXPECT(miner_rank_topk_subset(st, F16, W, buf, buf, buf, 0, 1000, 768, 64, 10, ib, 4, wb, ib, 5, fo, io, nullptr, 0), MINER_OK);
  EXPECT(miner_rank_topk_subset(st, F16, W, buf, buf, buf, 0, 1000, 768, 64, 10, nullptr, 0, nullptr, nullptr, 0, fo, io, nullptr, 0), MINER_OK);
  EXPECT(miner_rank_topk_subset(st, F16, MINER_SCORE_MAX, buf, nullptr, buf, 0, 1000, 768, 64, 256, ib, 256, wb, (const int32_t*)mis, 2147483647, fo, io, buf, 0), MINER_OK);

  // ---- miner_topk_merge ----
  EXPECT(miner_topk_merge(st, fb, ib, 10, fb, ib, 10, -1, 10, nullptr, 0, fo, io), MINER_EINVAL);
  EXPECT(miner_topk_merge(st, fb, ib, -1, fb, ib, 10, 4, 10, nullptr, 0, fo, io), MINER_EINVAL);
  EXPECT(miner_topk_merge(st, fb, ib, 10, fb, ib, -1, 4, 10, nullptr, 0, fo, io), MINER_EINVAL);
  EXPECT(miner_topk_merge(st, fb, ib, 10, fb, ib, 10, 4, 0, nullptr, 0, fo, io), MINER_EINVAL);
  EXPECT(miner_topk_merge(st, fb, ib, 10, fb, ib, 10, 4, -2147483647 - 1, nullptr, 0, fo, io), MINER_EINVAL);
  EXPECT(miner_topk_merge(st, fb, ib, 257, fb, ib, 10, 4, 10, nullptr, 0, fo, io), MINER_ESHAPE);
  EXPECT(miner_topk_merge(st, fb, ib, 10, fb, ib, 2147483647, 4, 10, nullptr, 0, fo, io), MINER_ESHAPE);
  EXPECT(miner_topk_merge(st, fb, ib, 10, fb, ib, 10, 4, 257, nullptr, 0, fo, io), MINER_ESHAPE);
  EXPECT(miner_topk_merge(st, nullptr, ib, 10, fb, ib, 10, 4, 10, nullptr, 0, fo, io), MINER_EINVAL);
  EXPECT(miner_topk_merge(st, fb, nullptr, 10, fb, ib, 10, 4, 10, nullptr, 0, fo, io), MINER_EINVAL);
  EXPECT(miner_topk_merge(st, fb, ib, 10, nullptr, ib, 10, 4, 10, nullptr, 0, fo, io), MINER_EINVAL);
  EXPECT(miner_topk_merge(st, fb, ib, 10, fb, nullptr, 10, 4, 10, nullptr, 0, fo, io), MINER_EINVAL);
  EXPECT(miner_topk_merge(st, fb, ib, 10, fb, ib, 10, 4, 10, nullptr, 0, nullptr, io), MINER_EINVAL);
  EXPECT(miner_topk_merge(st, fb, ib, 10, fb, ib, 10, 4, 10, nullptr, 0, fo, nullptr), MINER_EINVAL);
  EXPECT(miner_topk_merge(st, fb, ib, 10, fb, ib, 10, 4, 10, wb, 0, fo, io), MINER_EINVAL);
  EXPECT(miner_topk_merge(st, fb, ib, 10, fb, ib, 10, 4, 10, wb, -3, fo, io), MINER_EINVAL);
  EXPECT(miner_topk_merge(st, fodd, ib, 10, fb, ib, 10, 4, 10, nullptr, 0, fo, io), MINER_EALIGN);
  EXPECT(miner_topk_merge(st, fb, iodd, 10, fb, ib, 10, 4, 10, nullptr, 0, fo, io), MINER_EALIGN);
  EXPECT(miner_topk_merge(st, fb, ib, 10, fodd, ib, 10, 4, 10, nullptr, 0, fo, io), MINER_EALIGN);
  EXPECT(miner_topk_merge(st, fb, ib, 10, fb, iodd, 10, 4, 10, nullptr, 0, fo, io), MINER_EALIGN);
  EXPECT(miner_topk_merge(st, fb, ib, 10, fb, ib, 10, 4, 10, wodd, 1000, fo, io), MINER_EALIGN);
  EXPECT(miner_topk_merge(st, fb, ib, 10, fb, ib, 10, 4, 10, nullptr, 0, foodd, io), MINER_EALIGN);
  EXPECT(miner_topk_merge(st, fb, ib, 10, fb, ib, 10, 4, 10, nullptr, 0, fo, ioodd), MINER_EALIGN);
  // accepted: U == 0 returns after the validation; an empty list needs no pointers
  EXPECT(miner_topk_merge(st, fb, ib, 256, fb, ib, 256, 0, 256, wb, 1000, fo, io), MINER_OK);
  EXPECT(miner_topk_merge(st, nullptr, nullptr, 0, nullptr, nullptr, 0, 0, 1, nullptr, 0, fo, io), MINER_OK);

  printf("abi_errors_subset: %d calls, %d failures\n", g_calls, g_fail);
  return g_fail ? 1 : 0;
}
