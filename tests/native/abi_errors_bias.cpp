// Host-side argument validation of miner_rank_topk_biased, miner_score_pairs_biased and
// miner_rank_count_biased (include/miner_corpus.h), built like abi_errors_rank.cpp (host code under
// AddressSanitizer, miner_amd/build.py --asan) and run on a CPU-only machine by
// tests/test_corpus_bias_host.py: the prior table's checks return their documented MINER_E* codes
// after the unbiased call's own checks and before any device work, the accepted argument sets return
// MINER_OK with U = 0 or C = 0 (an empty id list, M = 0, with U = 0: with users it fills the lists),
// so nothing launches, and ASan must report nothing. The pointers are host addresses that a correct validation never
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
  const int32_t* iodd = (const int32_t*)(g_buf + 2);
  const uint32_t* wb = (const uint32_t*)g_buf;
  const float* fb = (const float*)g_buf;
  const float* fodd = (const float*)(g_buf + 2);
  float* fo = (float*)(g_buf + 1024);
  int32_t* io = (int32_t*)(g_buf + 2048);
  void* st = nullptr;
  const int F16 = MINER_DTYPE_F16, W = MINER_SCORE_WEIGHTED;

  if (miner_abi_version() != MINER_ABI_VERSION || MINER_ABI_VERSION != 6) { fprintf(stderr, "FAIL abi version\n"); ++g_fail; }

  // ---- miner_rank_topk_biased: the prior's checks, table form (news_ids NULL, M < 0) and subset form ----
  EXPECT(miner_rank_topk_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, fb, 0, nullptr), MINER_EINVAL);
  EXPECT(miner_rank_topk_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, fb, -2, ib), MINER_EINVAL);
  EXPECT(miner_rank_topk_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, nullptr, 1, ib), MINER_EINVAL);
  EXPECT(miner_rank_topk_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, nullptr, 0, ib), MINER_EINVAL);
  EXPECT(miner_rank_topk_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, fodd, 1, nullptr), MINER_EALIGN);
  EXPECT(miner_rank_topk_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, fb, 2, iodd), MINER_EALIGN);
  EXPECT(miner_rank_topk_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, ib, 5, fo, io, nullptr, 0, fodd, 1, nullptr), MINER_EALIGN);
  EXPECT(miner_rank_topk_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, ib, 5, fo, io, nullptr, 0, fodd, 0, iodd), MINER_EINVAL);   // G before the alignment
  // the older checks first, each with a bad prior as well
  EXPECT(miner_rank_topk_biased(st, 9, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, fodd, 1, nullptr), MINER_EINVAL);
  EXPECT(miner_rank_topk_biased(st, F16, W, buf, buf, buf, 4, 1000, 100, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, fb, 0, nullptr), MINER_ESHAPE);
  EXPECT(miner_rank_topk_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 257, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, fb, 0, nullptr), MINER_ESHAPE);
  EXPECT(miner_rank_topk_biased(st, F16, W, mis, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, fb, 0, nullptr), MINER_EALIGN);
  EXPECT(miner_rank_topk_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 257, wb, nullptr, -1, fo, io, nullptr, 0, fb, 0, nullptr), MINER_ESHAPE);
  EXPECT(miner_rank_topk_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 100, iodd, 3, wb, nullptr, -1, fo, io, nullptr, 0, fb, 0, nullptr), MINER_EALIGN);
  // the subset rules: a list pointer with M < 0, a length without a list, a misaligned list
  EXPECT(miner_rank_topk_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, ib, -1, fo, io, nullptr, 0, fb, 1, nullptr), MINER_EINVAL);
  EXPECT(miner_rank_topk_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, nullptr, 5, fo, io, nullptr, 0, fb, 1, nullptr), MINER_EINVAL);
  EXPECT(miner_rank_topk_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, iodd, 5, fo, io, nullptr, 0, fb, 0, nullptr), MINER_EALIGN);
  // accepted argument sets: U == 0 returns after the validation, with and without a prior
  EXPECT(miner_rank_topk_biased(st, F16, W, buf, buf, buf, 0, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, fb, 1, nullptr), MINER_OK);
  EXPECT(miner_rank_topk_biased(st, F16, W, buf, buf, buf, 0, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, fb, 3, ib), MINER_OK);
  EXPECT(miner_rank_topk_biased(st, F16, W, buf, buf, buf, 0, 1000, 768, 64, 100, nullptr, 0, nullptr, ib, 5, fo, io, nullptr, 0, (const float*)mis, 2147483647, (const int32_t*)mis), MINER_OK);
  EXPECT(miner_rank_topk_biased(st, F16, W, buf, buf, buf, 0, 1000, 768, 64, 100, nullptr, 0, nullptr, nullptr, 0, fo, io, nullptr, 0, fb, 1, nullptr), MINER_OK);
  EXPECT(miner_rank_topk_biased(st, F16, W, buf, buf, buf, 0, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, nullptr, 0, nullptr), MINER_OK);
  EXPECT(miner_rank_topk_biased(st, F16, W, buf, buf, buf, 0, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, nullptr, 7, nullptr), MINER_OK);   // G is read only with a table

  // ---- miner_score_pairs_biased ----
  EXPECT(miner_score_pairs_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, ib, 5, fo, fb, 0, nullptr), MINER_EINVAL);
  EXPECT(miner_score_pairs_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, ib, 5, fo, nullptr, 1, ib), MINER_EINVAL);
  EXPECT(miner_score_pairs_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, ib, 5, fo, fodd, 1, nullptr), MINER_EALIGN);
  EXPECT(miner_score_pairs_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, ib, 5, fo, fb, 1, iodd), MINER_EALIGN);
  EXPECT(miner_score_pairs_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, ib, 0, fo, fb, 0, nullptr), MINER_EINVAL);   // before the C == 0 return
  EXPECT(miner_score_pairs_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, ib, -1, fo, fodd, 1, nullptr), MINER_EINVAL);  // C first
  EXPECT(miner_score_pairs_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, iodd, 5, fo, fb, 0, nullptr), MINER_EALIGN);   // the id list first
  EXPECT(miner_score_pairs_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 65, ib, 5, fo, fb, 0, nullptr), MINER_ESHAPE);
  EXPECT(miner_score_pairs_biased(st, F16, W, buf, buf, buf, 0, 1000, 768, 64, ib, 5, fo, fb, 2, ib), MINER_OK);
  EXPECT(miner_score_pairs_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, ib, 0, fo, fb, 1, nullptr), MINER_OK);
  EXPECT(miner_score_pairs_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, nullptr, 0, nullptr, nullptr, 0, nullptr), MINER_OK);

  // ---- miner_rank_count_biased ----
  EXPECT(miner_rank_count_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, fb, ib, 3, wb, io, fb, 0, nullptr), MINER_EINVAL);
  EXPECT(miner_rank_count_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, fb, ib, 3, wb, io, nullptr, 2, ib), MINER_EINVAL);
  EXPECT(miner_rank_count_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, fb, ib, 3, wb, io, fodd, 1, nullptr), MINER_EALIGN);
  EXPECT(miner_rank_count_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, fb, ib, 3, wb, io, fb, 1, iodd), MINER_EALIGN);
  EXPECT(miner_rank_count_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, fb, ib, 65, wb, io, fb, 0, nullptr), MINER_ESHAPE);   // the cap first
  EXPECT(miner_rank_count_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, fodd, ib, 3, wb, io, fb, 0, nullptr), MINER_EALIGN);  // the targets first
  EXPECT(miner_rank_count_biased(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, fb, ib, 0, wb, io, fodd, 1, nullptr), MINER_EINVAL);
  EXPECT(miner_rank_count_biased(st, F16, W, buf, buf, buf, 0, 1000, 768, 64, fb, ib, 3, wb, io, fb, 1, nullptr), MINER_OK);
  EXPECT(miner_rank_count_biased(st, F16, W, buf, buf, buf, 0, 1000, 768, 64, fb, ib, 64, nullptr, io, fb, 4, ib), MINER_OK);
  EXPECT(miner_rank_count_biased(st, F16, W, buf, buf, buf, 0, 1000, 768, 64, fb, ib, 3, wb, io, nullptr, 0, nullptr), MINER_OK);

  printf("abi_errors_bias: %d calls, %d failures\n", g_calls, g_fail);
  return g_fail ? 1 : 0;
}
