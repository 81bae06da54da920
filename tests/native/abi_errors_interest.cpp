// Host-side argument validation of miner_score_pairs_interest, miner_rank_topk_interest and
// miner_topk_merge_grouped (include/miner_corpus.h), built like abi_errors_cap.cpp (host code under
// AddressSanitizer, miner_amd/build.py --asan) and run on a CPU-only machine by
// tests/test_corpus_interest_host.py: the new checks return their documented MINER_E* codes after
// the base call's own checks, in the documented order, and before any device work; the accepted
// argument sets return MINER_OK with U = 0, so nothing launches; and ASan must report nothing. The
// pointers are host addresses that a correct validation never dereferences: `buf` is 16-byte aligned,
// `mis` is 4-byte but not 16-byte aligned, the `odd` ones are not 4-byte aligned.
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
  int32_t* go = (int32_t*)(g_buf + 3072);
  int32_t* gmis = (int32_t*)(g_buf + 3076);
  int32_t* godd = (int32_t*)(g_buf + 3074);
  void* st = nullptr;
  const int F16 = MINER_DTYPE_F16, W = MINER_SCORE_WEIGHTED, MX = MINER_SCORE_MAX, MEAN = MINER_SCORE_MEAN;

  if (miner_abi_version() != MINER_ABI_VERSION || MINER_ABI_VERSION != 6) { fprintf(stderr, "FAIL abi version\n"); ++g_fail; }

  // ---- miner_score_pairs_interest: the interests' checks, with users (no launch) and without ----
  for (int U = 0; U <= 4; U += 4) {
    EXPECT(miner_score_pairs_interest(st, F16, MEAN, buf, buf, buf, U, 1000, 768, 64, ib, 10, fo, nullptr, 0, nullptr, go), MINER_EINVAL);
    EXPECT(miner_score_pairs_interest(st, F16, W, buf, buf, buf, U, 1000, 768, 64, ib, 10, fo, nullptr, 0, nullptr, godd), MINER_EALIGN);
    EXPECT(miner_score_pairs_interest(st, F16, MEAN, buf, buf, buf, U, 1000, 768, 64, ib, 10, fo, nullptr, 0, nullptr, godd), MINER_EINVAL);   // the score type before the alignment
    EXPECT(miner_score_pairs_interest(st, F16, MX, buf, nullptr, buf, U, 1000, 768, 64, ib, 10, fo, fb, 2, ib, godd), MINER_EALIGN);
  }
  // the biased call's checks first, each with bad interests as well
  EXPECT(miner_score_pairs_interest(st, 9, MEAN, buf, buf, buf, 4, 1000, 768, 64, ib, 10, fo, nullptr, 0, nullptr, godd), MINER_EINVAL);
  EXPECT(miner_score_pairs_interest(st, F16, MEAN, buf, buf, buf, 4, 1000, 100, 64, ib, 10, fo, nullptr, 0, nullptr, godd), MINER_ESHAPE);
  EXPECT(miner_score_pairs_interest(st, F16, MEAN, mis, buf, buf, 4, 1000, 768, 64, ib, 10, fo, nullptr, 0, nullptr, godd), MINER_EALIGN);
  EXPECT(miner_score_pairs_interest(st, F16, MEAN, buf, buf, buf, 4, 1000, 768, 64, ib, -1, fo, nullptr, 0, nullptr, godd), MINER_EINVAL);
  EXPECT(miner_score_pairs_interest(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, iodd, 10, fo, nullptr, 0, nullptr, go), MINER_EALIGN);
  EXPECT(miner_score_pairs_interest(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, ib, 10, fo, fb, 0, nullptr, godd), MINER_EINVAL);      // the prior first
  EXPECT(miner_score_pairs_interest(st, F16, MEAN, buf, buf, buf, 4, 1000, 768, 64, ib, 10, fo, fodd, 1, nullptr, go), MINER_EALIGN);  // the prior's alignment first
  // accepted argument sets: U == 0 / C == 0 return after the validation
  EXPECT(miner_score_pairs_interest(st, F16, W, buf, buf, buf, 0, 1000, 768, 64, ib, 10, fo, nullptr, 0, nullptr, go), MINER_OK);
  EXPECT(miner_score_pairs_interest(st, F16, MX, buf, nullptr, buf, 0, 1000, 768, 64, ib, 10, fo, fb, 3, ib, gmis), MINER_OK);
  EXPECT(miner_score_pairs_interest(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, nullptr, 0, nullptr, nullptr, 0, nullptr, go), MINER_OK);
  EXPECT(miner_score_pairs_interest(st, F16, MEAN, buf, buf, buf, 0, 1000, 768, 64, ib, 10, fo, nullptr, 0, nullptr, nullptr), MINER_OK);  // no interests: the biased call

  // ---- miner_rank_topk_interest ----
#define RANK(stype, U, clus, cap, as, ai, icap, tg) \
  miner_rank_topk_interest(st, F16, stype, buf, buf, buf, U, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, \
                           nullptr, 0, nullptr, clus, cap, as, ai, icap, tg)
  for (int U = 0; U <= 4; U += 4) {
    EXPECT(RANK(W, U, nullptr, 0, nullptr, nullptr, -1, go), MINER_EINVAL);
    EXPECT(RANK(W, U, nullptr, 0, nullptr, nullptr, 257, go), MINER_ESHAPE);
    EXPECT(RANK(W, U, ib, 2, nullptr, nullptr, 2, go), MINER_EINVAL);            // never with a cluster table
    EXPECT(RANK(W, U, nullptr, 0, fb, ib, 2, go), MINER_EINVAL);                 // no cursor under caps
    EXPECT(RANK(MEAN, U, nullptr, 0, nullptr, nullptr, 2, go), MINER_EINVAL);    // no dominant interest
    EXPECT(RANK(W, U, nullptr, 0, nullptr, nullptr, 0, go), MINER_EINVAL);       // the interests only under a cap
    EXPECT(RANK(W, U, nullptr, 0, nullptr, nullptr, 2, godd), MINER_EALIGN);
    // the order: the cap's range, the combinations, the score type, the output, its alignment
    EXPECT(RANK(MEAN, U, ib, 2, nullptr, nullptr, 257, godd), MINER_ESHAPE);
    EXPECT(RANK(MEAN, U, nullptr, 0, nullptr, nullptr, -3, godd), MINER_EINVAL);
    EXPECT(RANK(MEAN, U, nullptr, 0, nullptr, nullptr, 2, godd), MINER_EINVAL);
    EXPECT(RANK(W, U, nullptr, 0, nullptr, nullptr, 0, godd), MINER_EINVAL);
  }
  // miner_rank_topk_after's checks first, each with bad interest arguments as well
  EXPECT(miner_rank_topk_interest(st, 9, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, -1, godd), MINER_EINVAL);
  EXPECT(miner_rank_topk_interest(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 257, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, -1, godd), MINER_ESHAPE);
  EXPECT(miner_rank_topk_interest(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 257, wb, nullptr, -1, fo, io, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, -1, godd), MINER_ESHAPE);
  EXPECT(miner_rank_topk_interest(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, iodd, 5, fo, io, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, -1, godd), MINER_EALIGN);
  EXPECT(miner_rank_topk_interest(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, fb, 0, nullptr, nullptr, 0, nullptr, nullptr, 257, godd), MINER_EINVAL);  // the prior
  EXPECT(miner_rank_topk_interest(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, nullptr, 0, nullptr, ib, 0, nullptr, nullptr, 257, godd), MINER_EINVAL);   // the cluster cap
  EXPECT(miner_rank_topk_interest(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, fb, nullptr, 257, godd), MINER_EINVAL);  // half a cursor
  EXPECT(miner_rank_topk_interest(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, nullptr, 0, nullptr, ib, 2, fb, ib, 257, godd), MINER_EINVAL);           // a cursor under cluster caps
  EXPECT(miner_rank_topk_interest(st, F16, W, buf, buf, buf, 4, 1000, 768, 64, 100, ib, 3, wb, nullptr, -1, fo, io, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, fodd, ib, -1, godd), MINER_EALIGN);       // the cursor's alignment
  // accepted argument sets: U == 0 returns after the validation
  EXPECT(RANK(W, 0, nullptr, 0, nullptr, nullptr, 1, go), MINER_OK);
  EXPECT(RANK(MX, 0, nullptr, 0, nullptr, nullptr, 256, gmis), MINER_OK);
  EXPECT(RANK(W, 0, nullptr, 0, nullptr, nullptr, 3, nullptr), MINER_OK);       // the interests are optional
  EXPECT(RANK(W, 0, nullptr, 0, nullptr, nullptr, 0, nullptr), MINER_OK);       // neither: miner_rank_topk_after
  EXPECT(RANK(MEAN, 0, ib, 2, nullptr, nullptr, 0, nullptr), MINER_OK);
  EXPECT(RANK(MEAN, 0, nullptr, 0, fb, ib, 0, nullptr), MINER_OK);
  EXPECT(miner_rank_topk_interest(st, F16, W, buf, buf, buf, 0, 1000, 768, 64, 100, nullptr, 0, nullptr, ib, 5, fo, io, buf, 64, fb, 3, ib, nullptr, 0, nullptr, nullptr, 2, go), MINER_OK);   // subset, prior, a workspace

  // ---- miner_topk_merge_grouped ----
  for (int U = 0; U <= 4; U += 4) {
    EXPECT(miner_topk_merge_grouped(st, fb, ib, 100, fb, ib, 100, U, 100, wb, 1000, fo, io, ib, ib, go, -1), MINER_EINVAL);
    EXPECT(miner_topk_merge_grouped(st, fb, ib, 100, fb, ib, 100, U, 100, wb, 1000, fo, io, ib, ib, go, 257), MINER_ESHAPE);
    EXPECT(miner_topk_merge_grouped(st, fb, ib, 100, fb, ib, 100, U, 100, wb, 1000, fo, io, nullptr, ib, go, 2), MINER_EINVAL);
    EXPECT(miner_topk_merge_grouped(st, fb, ib, 100, fb, ib, 100, U, 100, wb, 1000, fo, io, ib, nullptr, go, 2), MINER_EINVAL);
    EXPECT(miner_topk_merge_grouped(st, fb, ib, 100, fb, ib, 100, U, 100, wb, 1000, fo, io, ib, ib, nullptr, 0), MINER_EINVAL);
    EXPECT(miner_topk_merge_grouped(st, fb, ib, 100, fb, ib, 100, U, 100, nullptr, 0, fo, io, iodd, ib, go, 2), MINER_EALIGN);
    EXPECT(miner_topk_merge_grouped(st, fb, ib, 100, fb, ib, 100, U, 100, nullptr, 0, fo, io, ib, iodd, go, 2), MINER_EALIGN);
    EXPECT(miner_topk_merge_grouped(st, fb, ib, 100, fb, ib, 100, U, 100, nullptr, 0, fo, io, ib, ib, godd, 0), MINER_EALIGN);
    EXPECT(miner_topk_merge_grouped(st, fb, ib, 100, fb, ib, 100, U, 100, nullptr, 0, fo, io, nullptr, iodd, godd, 2), MINER_EINVAL);   // NULL before the alignment
    EXPECT(miner_topk_merge_grouped(st, fb, ib, 100, fb, ib, 100, U, 100, nullptr, 0, fo, io, nullptr, iodd, godd, 257), MINER_ESHAPE); // cap before the pointers
  }
  // the base call's checks first, each with bad groups as well
  EXPECT(miner_topk_merge_grouped(st, fb, ib, -1, fb, ib, 100, 4, 100, wb, 1000, fo, io, nullptr, iodd, godd, -1), MINER_EINVAL);
  EXPECT(miner_topk_merge_grouped(st, fb, ib, 257, fb, ib, 100, 4, 100, wb, 1000, fo, io, nullptr, iodd, godd, -1), MINER_ESHAPE);
  EXPECT(miner_topk_merge_grouped(st, fb, ib, 100, fb, ib, 100, 4, 0, wb, 1000, fo, io, nullptr, iodd, godd, -1), MINER_EINVAL);
  EXPECT(miner_topk_merge_grouped(st, fb, nullptr, 100, fb, ib, 100, 4, 100, wb, 1000, fo, io, nullptr, iodd, godd, 257), MINER_EINVAL);
  EXPECT(miner_topk_merge_grouped(st, fb, ib, 100, fb, ib, 100, 4, 100, wb, 0, fo, io, nullptr, iodd, godd, 257), MINER_EINVAL);   // a bitmap with N <= 0
  EXPECT(miner_topk_merge_grouped(st, fodd, ib, 100, fb, ib, 100, 4, 100, wb, 1000, fo, io, ib, ib, go, 257), MINER_EALIGN);
  // accepted argument sets
  EXPECT(miner_topk_merge_grouped(st, fb, ib, 100, fb, ib, 100, 0, 100, wb, 1000, fo, io, ib, ib, go, 0), MINER_OK);
  EXPECT(miner_topk_merge_grouped(st, fb, ib, 100, fb, ib, 100, 0, 100, nullptr, 0, fo, io, ib, ib, gmis, 256), MINER_OK);
  EXPECT(miner_topk_merge_grouped(st, nullptr, nullptr, 0, fb, ib, 256, 0, 256, nullptr, 0, fo, io, nullptr, ib, go, 1), MINER_OK);   // ka == 0: no a_groups
  EXPECT(miner_topk_merge_grouped(st, fb, ib, 7, nullptr, nullptr, 0, 0, 7, nullptr, 0, fo, io, ib, nullptr, go, 0), MINER_OK);

  printf("abi_errors_interest: %d calls, %d failures\n", g_calls, g_fail);
  return g_fail ? 1 : 0;
}
