// Host-side argument validation of miner_score_pairs and miner_rank_count (include/miner_corpus.h),
// built like abi_errors.cpp (host code under AddressSanitizer, miner_amd/build.py --asan) and run on
// a CPU-only machine by tests/test_corpus_rank_host.py: every error path of the two entry points
// returns its documented MINER_E* code before any device work, the accepted argument sets return
// MINER_OK with U = 0 or C = 0 (nothing launches), and ASan must report nothing. The pointers are
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
  if (MINER_CORPUS_MAX_TARGETS != 64) { fprintf(stderr, "FAIL MINER_CORPUS_MAX_TARGETS\n"); ++g_fail; }

  // ---- miner_score_pairs: its own checks ----
  EXPECT(miner_score_pairs(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, ib, -1, fo), MINER_EINVAL);
  EXPECT(miner_score_pairs(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, ib, -2147483647 - 1, fo), MINER_EINVAL);
  EXPECT(miner_score_pairs(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, nullptr, 5, fo), MINER_EINVAL);
  EXPECT(miner_score_pairs(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, ib, 5, nullptr), MINER_EINVAL);
  EXPECT(miner_score_pairs(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, iodd, 5, fo), MINER_EALIGN);
  EXPECT(miner_score_pairs(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, ib, 5, foodd), MINER_EALIGN);
  EXPECT(miner_score_pairs(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, iodd, 0, fo), MINER_EALIGN);
  // ---- the shared checks first, with their codes (each with a bad id list as well) ----
  EXPECT(miner_score_pairs(st, 9, W, buf, buf, buf, 4, 1000, 768, 64, nullptr, -1, fo), MINER_EINVAL);
  EXPECT(miner_score_pairs(st, F16, W, buf, buf, buf, 4, 1000, 100, 64, iodd, 5, fo), MINER_ESHAPE);
  EXPECT(miner_score_pairs(st, F16, W, buf, buf, buf, 4, 1000, 768, 65, iodd, 5, fo), MINER_ESHAPE);
  EXPECT(miner_score_pairs(st, F16, W, buf, buf, buf, 4, 1000, 768, 0, iodd, 5, fo), MINER_EINVAL);
  EXPECT(miner_score_pairs(st, F16, 7, buf, buf, buf, 4, 1000, 768, 64, iodd, 5, fo), MINER_EINVAL);
  EXPECT(miner_score_pairs(st, F16, W, buf, buf, buf, -1, 1000, 768, 64, iodd, 5, fo), MINER_EINVAL);
  EXPECT(miner_score_pairs(st, F16, W, buf, buf, buf, 4, 0, 768, 64, iodd, 5, fo), MINER_EINVAL);
  EXPECT(miner_score_pairs(st, F16, W, nullptr, buf, buf, 4, 1000, 768, 64, iodd, 5, fo), MINER_EINVAL);
  EXPECT(miner_score_pairs(st, F16, W, buf, nullptr, buf, 4, 1000, 768, 64, iodd, 5, fo), MINER_EINVAL);
  EXPECT(miner_score_pairs(st, F16, W, buf, buf, nullptr, 4, 1000, 768, 64, iodd, 5, fo), MINER_EINVAL);
  EXPECT(miner_score_pairs(st, F16, W, mis, buf, buf, 4, 1000, 768, 64, nullptr, 5, fo), MINER_EALIGN);
  EXPECT(miner_score_pairs(st, F16, W, buf, mis, buf, 4, 1000, 768, 64, nullptr, 5, fo), MINER_EALIGN);
  EXPECT(miner_score_pairs(st, F16, W, buf, buf, mis, 4, 1000, 768, 64, nullptr, 5, fo), MINER_EALIGN);
  // ---- accepted argument sets: U == 0 or C == 0 returns after the validation ----
  EXPECT(miner_score_pairs(st, F16, W, buf, buf, buf, 0, 1000, 768, 64, ib, 5, fo), MINER_OK);
  EXPECT(miner_score_pairs(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, ib, 0, fo), MINER_OK);
  EXPECT(miner_score_pairs(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, nullptr, 0, nullptr), MINER_OK);
  EXPECT(miner_score_pairs(st, F16, MINER_SCORE_MAX, buf, nullptr, buf, 0, 1000, 768, 64, (const int32_t*)mis, 2147483647, (float*)mis), MINER_OK);
  EXPECT(miner_score_pairs(st, MINER_DTYPE_F32, MINER_SCORE_MEAN, buf, nullptr, buf, 0, 1, 32, 1, ib, 1, fo), MINER_OK);

  // ---- miner_rank_count: its own checks ----
  EXPECT(miner_rank_count(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, fb, ib, 0, wb, io), MINER_EINVAL);
  EXPECT(miner_rank_count(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, fb, ib, -3, wb, io), MINER_EINVAL);
  EXPECT(miner_rank_count(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, nullptr, ib, 3, wb, io), MINER_EINVAL);
  EXPECT(miner_rank_count(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, fb, nullptr, 3, wb, io), MINER_EINVAL);
  EXPECT(miner_rank_count(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, fb, ib, 3, wb, nullptr), MINER_EINVAL);
  EXPECT(miner_rank_count(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, fb, ib, 65, wb, io), MINER_ESHAPE);
  EXPECT(miner_rank_count(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, fb, ib, 2147483647, nullptr, io), MINER_ESHAPE);
  EXPECT(miner_rank_count(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, fodd, ib, 3, wb, io), MINER_EALIGN);
  EXPECT(miner_rank_count(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, fb, iodd, 3, wb, io), MINER_EALIGN);
  EXPECT(miner_rank_count(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, fb, ib, 3, wodd, io), MINER_EALIGN);
  EXPECT(miner_rank_count(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, fb, ib, 3, wb, ioodd), MINER_EALIGN);
  EXPECT(miner_rank_count(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, fodd, ib, 65, wb, io), MINER_ESHAPE);   // the shape before the alignment
  EXPECT(miner_rank_count(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, nullptr, ib, 65, wb, io), MINER_EINVAL);  // the NULL before the shape
  // ---- the shared checks first ----
  EXPECT(miner_rank_count(st, 9, W, buf, buf, buf, 4, 1000, 768, 64, fb, ib, 0, wb, io), MINER_EINVAL);
  EXPECT(miner_rank_count(st, F16, W, buf, buf, buf, 4, 1000, 100, 64, fodd, ib, 3, wb, io), MINER_ESHAPE);
  EXPECT(miner_rank_count(st, F16, W, buf, buf, buf, 4, 1000, 768, 65, fodd, ib, 3, wb, io), MINER_ESHAPE);
  EXPECT(miner_rank_count(st, F16, 7, buf, buf, buf, 4, 1000, 768, 64, fodd, ib, 3, wb, io), MINER_EINVAL);
  EXPECT(miner_rank_count(st, F16, W, buf, buf, buf, -1, 1000, 768, 64, fodd, ib, 3, wb, io), MINER_EINVAL);
  EXPECT(miner_rank_count(st, F16, W, buf, buf, buf, 4, 0, 768, 64, fodd, ib, 3, wb, io), MINER_EINVAL);
  EXPECT(miner_rank_count(st, F16, W, nullptr, buf, buf, 4, 1000, 768, 64, fodd, ib, 3, wb, io), MINER_EINVAL);
  EXPECT(miner_rank_count(st, F16, W, buf, nullptr, buf, 4, 1000, 768, 64, fodd, ib, 3, wb, io), MINER_EINVAL);
  EXPECT(miner_rank_count(st, F16, W, buf, buf, nullptr, 4, 1000, 768, 64, fodd, ib, 3, wb, io), MINER_EINVAL);
  EXPECT(miner_rank_count(st, F16, W, mis, buf, buf, 4, 1000, 768, 64, fb, ib, 65, wb, io), MINER_EALIGN);
  EXPECT(miner_rank_count(st, F16, W, buf, mis, buf, 4, 1000, 768, 64, fb, ib, 65, wb, io), MINER_EALIGN);
  EXPECT(miner_rank_count(st, F16, W, buf, buf, mis, 4, 1000, 768, 64, fb, ib, 65, wb, io), MINER_EALIGN);
  // ---- accepted argument sets: U == 0 returns after the validation ----
  EXPECT(miner_rank_count(st, F16, W, buf, buf, buf, 0, 1000, 768, 64, fb, ib, 1, wb, io), MINER_OK);
  EXPECT(miner_rank_count(st, F16, W, buf, buf, buf, 0, 1000, 768, 64, fb, ib, 64, nullptr, io), MINER_OK);
  EXPECT(miner_rank_count(st, F16, MINER_SCORE_MAX, buf, nullptr, buf, 0, 1000, 768, 64, (const float*)mis, (const int32_t*)mis, 64, (const uint32_t*)mis, (int32_t*)mis), MINER_OK);

  printf("abi_errors_rank: %d calls, %d failures\n", g_calls, g_fail);
  return g_fail ? 1 : 0;
}
