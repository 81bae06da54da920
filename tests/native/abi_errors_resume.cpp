// Host-side argument validation of miner_rank_topk_resume and miner_walk_advance
// (include/miner_corpus.h), built like abi_errors_after.cpp (host code under AddressSanitizer,
// miner_amd/build.py --asan) and run on a CPU-only machine by tests/test_corpus_resume_host.py: the new
// checks return their documented MINER_E* codes after miner_rank_topk_interest's own checks and
// before any device work, the accepted argument sets return MINER_OK with U = 0, so nothing launches,
// and ASan must report nothing. The pointers are host addresses that a correct validation never
// dereferences: `buf` is 16-byte aligned, the `mis` ones 4-byte but not 16-byte aligned, the `odd`
// ones not 4-byte aligned.
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

static void* const st = nullptr;
static void* const buf = g_buf;
static const int32_t* const ib = (const int32_t*)g_buf;
static const int32_t* const imis = (const int32_t*)(g_buf + 4);
static const int32_t* const iodd = (const int32_t*)(g_buf + 2);
static const uint32_t* const wb = (const uint32_t*)g_buf;
static const float* const fb = (const float*)g_buf;
static const float* const fodd = (const float*)(g_buf + 2);
static float* const fo = (float*)(g_buf + 1024);
static int32_t* const io = (int32_t*)(g_buf + 2048);
static int32_t* const iood = (int32_t*)(g_buf + 2050);
static uint8_t* const bo = g_buf + 3072;
static const int F16 = MINER_DTYPE_F16, W = MINER_SCORE_WEIGHTED;

// miner_rank_topk_resume on config-5 shapes: what varies is the users, topk, the cluster table and
// its cap, the cursor, the interest cap and the state
static int resume(int U, int topk, const int32_t* clus, int cap, const float* as, const int32_t* ai, int icap, int32_t* tg,
                  const int32_t* ug, const int32_t* uc, const int32_t* un, int Q, int score = W, const void* mui = g_buf) {
  return miner_rank_topk_resume(st, F16, score, mui, buf, buf, U, 1000, 768, 64, topk, ib, 3, wb, nullptr, -1, fo, io,
                                nullptr, 0, nullptr, 0, nullptr, clus, cap, as, ai, icap, tg, ug, uc, un, Q);
}

static int advance(const float* ps, const int32_t* pi, const int32_t* pg, const int32_t* clus, int nc, const int32_t* ig,
                   const int32_t* ic, const int32_t* in, int Qin, float* oas, int32_t* oai, int32_t* og, int32_t* oc,
                   int32_t* on, uint8_t* ov, int U, int k, int Q) {
  return miner_walk_advance(st, ps, pi, pg, clus, nc, ig, ic, in, Qin, oas, oai, og, oc, on, ov, U, k, Q);
}

int main() {
  if (miner_abi_version() != MINER_ABI_VERSION || MINER_ABI_VERSION != 6) { fprintf(stderr, "FAIL abi version\n"); ++g_fail; }
  const int QM = MINER_CORPUS_MAX_WALK_GROUPS;

  for (int U = 0; U <= 4; U += 4) {
    // ---- no table: miner_rank_topk_interest's answers, a cursor under caps still refused ----
    EXPECT(resume(U, 100, ib, 2, fb, ib, 0, nullptr, nullptr, nullptr, nullptr, 0), MINER_EINVAL);
    EXPECT(resume(U, 100, nullptr, 0, fb, ib, 3, nullptr, nullptr, nullptr, nullptr, 0), MINER_EINVAL);
    EXPECT(resume(U, 100, nullptr, 0, fodd, ib, 0, nullptr, nullptr, nullptr, nullptr, -7), MINER_EALIGN);   // Q is not read
    // ---- with a table: the new checks, in their order ----
    EXPECT(resume(U, 100, ib, 2, nullptr, nullptr, 0, nullptr, ib, ib, ib, 8), MINER_EINVAL);       // no cursor
    EXPECT(resume(U, 100, ib, 2, nullptr, nullptr, 0, nullptr, iodd, ib, ib, QM + 1), MINER_EINVAL);   // ... before shape and alignment
    EXPECT(resume(U, 100, nullptr, 0, fb, ib, 0, nullptr, ib, ib, ib, 8), MINER_EINVAL);            // no cap of either kind
    EXPECT(resume(U, 100, nullptr, 0, fb, ib, 0, nullptr, iodd, ib, ib, QM + 1), MINER_EINVAL);
    EXPECT(resume(U, 100, ib, 2, fb, ib, 3, nullptr, ib, ib, ib, 8), MINER_EINVAL);                 // both kinds of cap
    EXPECT(resume(U, 100, ib, 2, fb, ib, 0, nullptr, ib, ib, ib, -1), MINER_EINVAL);                // Q < 0
    EXPECT(resume(U, 100, ib, 2, fb, ib, 0, nullptr, nullptr, ib, ib, 8), MINER_EINVAL);            // a NULL among the three
    EXPECT(resume(U, 100, ib, 2, fb, ib, 0, nullptr, ib, nullptr, ib, 8), MINER_EINVAL);
    EXPECT(resume(U, 100, ib, 2, fb, ib, 0, nullptr, ib, ib, nullptr, 8), MINER_EINVAL);
    EXPECT(resume(U, 100, nullptr, 0, fb, ib, 3, nullptr, nullptr, nullptr, ib, QM + 1), MINER_EINVAL);   // ... before the shape
    EXPECT(resume(U, 100, ib, 2, fb, ib, 0, nullptr, ib, ib, ib, QM + 1), MINER_ESHAPE);            // Q past the limit
    EXPECT(resume(U, 100, ib, 2, fb, ib, 0, nullptr, iodd, ib, ib, QM + 1), MINER_ESHAPE);          // ... before the alignment
    EXPECT(resume(U, 100, ib, 2, fb, ib, 0, nullptr, iodd, ib, ib, 8), MINER_EALIGN);
    EXPECT(resume(U, 100, ib, 2, fb, ib, 0, nullptr, ib, iodd, ib, 8), MINER_EALIGN);
    EXPECT(resume(U, 100, nullptr, 0, fb, ib, 3, io, ib, ib, iodd, 8), MINER_EALIGN);
    // ---- the older checks first, each with a bad state as well ----
    EXPECT(resume(U, 257, ib, 2, fb, ib, 0, nullptr, ib, nullptr, ib, 8), MINER_ESHAPE);            // topk
    EXPECT(resume(U, 100, ib, 257, fb, ib, 0, nullptr, ib, nullptr, ib, 8), MINER_ESHAPE);          // the caps' checks
    EXPECT(resume(U, 100, iodd, 2, fb, ib, 0, nullptr, ib, nullptr, ib, 8), MINER_EALIGN);
    EXPECT(resume(U, 100, ib, 2, fb, nullptr, 0, nullptr, ib, ib, ib, 8), MINER_EINVAL);            // half a cursor
    EXPECT(resume(U, 100, ib, 2, fodd, ib, 0, nullptr, ib, nullptr, ib, 8), MINER_EALIGN);          // the cursor's alignment
    EXPECT(resume(U, 100, nullptr, 0, fb, ib, -1, nullptr, ib, nullptr, ib, 8), MINER_EINVAL);      // the interest cap's checks
    EXPECT(resume(U, 100, nullptr, 0, fb, ib, 257, nullptr, ib, nullptr, ib, 8), MINER_ESHAPE);
    EXPECT(resume(U, 100, nullptr, 0, fb, ib, 3, nullptr, ib, nullptr, ib, 8, MINER_SCORE_MEAN), MINER_EINVAL);
    EXPECT(resume(U, 100, ib, 2, fb, ib, 0, io, ib, nullptr, ib, 8), MINER_EINVAL);                 // interests without their cap
    EXPECT(resume(U, 100, nullptr, 0, fb, ib, 3, iood, ib, nullptr, ib, 8), MINER_EALIGN);
    EXPECT(resume(U, 100, ib, 2, fb, ib, 0, nullptr, ib, ib, ib, 8, W, g_buf + 4), MINER_EALIGN);   // the user vectors
  }
  // accepted argument sets: U == 0 returns after the validation
  EXPECT(resume(0, 100, ib, 2, fb, ib, 0, nullptr, ib, ib, ib, 8), MINER_OK);
  EXPECT(resume(0, 100, ib, 2, fb, ib, 0, nullptr, imis, imis, imis, QM), MINER_OK);                // 4-byte aligned, the limit
  EXPECT(resume(0, 100, ib, 2, fb, ib, 0, nullptr, ib, ib, ib, 0), MINER_OK);                       // an empty table
  EXPECT(resume(0, 100, nullptr, 0, fb, ib, 3, nullptr, ib, ib, ib, 64), MINER_OK);                 // the interest cap
  EXPECT(resume(0, 100, nullptr, 0, fb, ib, 3, io, ib, ib, ib, 64, MINER_SCORE_MAX), MINER_OK);
  EXPECT(resume(0, 100, ib, 2, fb, ib, 0, nullptr, ib, ib, ib, 8, MINER_SCORE_MEAN), MINER_OK);     // mean under cluster caps
  EXPECT(resume(0, 100, ib, 2, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0), MINER_OK);   // no table: the capped call
  EXPECT(resume(0, 100, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0), MINER_OK);

  // ---- miner_walk_advance ----
  for (int U = 0; U <= 4; U += 4) {
    EXPECT(advance(fb, ib, nullptr, ib, 100, ib, ib, ib, 8, fo, io, io, io, io, bo, -1, 10, 8), MINER_EINVAL);
    EXPECT(advance(fb, ib, nullptr, ib, 100, ib, ib, ib, 8, fo, io, io, io, io, bo, U, 0, 8), MINER_EINVAL);
    EXPECT(advance(fb, ib, nullptr, ib, 100, ib, ib, ib, 8, fo, io, io, io, io, bo, U, 10, -1), MINER_EINVAL);
    EXPECT(advance(fb, ib, nullptr, ib, 100, ib, ib, ib, -1, fo, io, io, io, io, bo, U, 10, 8), MINER_EINVAL);
    EXPECT(advance(fb, ib, nullptr, ib, 100, ib, ib, ib, 8, fo, io, io, io, io, bo, U, 0, QM + 1), MINER_EINVAL);   // before the shapes
    EXPECT(advance(fb, ib, nullptr, ib, 100, ib, ib, ib, 8, fo, io, io, io, io, bo, U, 257, 8), MINER_ESHAPE);
    EXPECT(advance(fb, ib, nullptr, ib, 100, ib, ib, ib, 8, fo, io, io, io, io, bo, U, 10, QM + 1), MINER_ESHAPE);
    EXPECT(advance(fb, ib, nullptr, ib, 100, ib, ib, ib, QM + 1, fo, io, io, io, io, bo, U, 10, 8), MINER_ESHAPE);
    EXPECT(advance(nullptr, ib, nullptr, ib, 100, ib, ib, ib, QM + 1, fo, io, io, io, io, bo, U, 10, 8), MINER_ESHAPE);   // before the pointers
    EXPECT(advance(nullptr, ib, nullptr, ib, 100, ib, ib, ib, 8, fo, io, io, io, io, bo, U, 10, 8), MINER_EINVAL);
    EXPECT(advance(fb, nullptr, nullptr, ib, 100, ib, ib, ib, 8, fo, io, io, io, io, bo, U, 10, 8), MINER_EINVAL);
    EXPECT(advance(fb, ib, nullptr, ib, 100, ib, ib, nullptr, 8, fo, io, io, io, io, bo, U, 10, 8), MINER_EINVAL);
    EXPECT(advance(fb, ib, nullptr, ib, 100, nullptr, ib, ib, 8, fo, io, io, io, io, bo, U, 10, 8), MINER_EINVAL);
    EXPECT(advance(fb, ib, nullptr, ib, 100, ib, nullptr, ib, 8, fo, io, io, io, io, bo, U, 10, 8), MINER_EINVAL);
    EXPECT(advance(fb, ib, nullptr, ib, 100, ib, ib, ib, 8, nullptr, io, io, io, io, bo, U, 10, 8), MINER_EINVAL);
    EXPECT(advance(fb, ib, nullptr, ib, 100, ib, ib, ib, 8, fo, nullptr, io, io, io, bo, U, 10, 8), MINER_EINVAL);
    EXPECT(advance(fb, ib, nullptr, ib, 100, ib, ib, ib, 8, fo, io, nullptr, io, io, bo, U, 10, 8), MINER_EINVAL);
    EXPECT(advance(fb, ib, nullptr, ib, 100, ib, ib, ib, 8, fo, io, io, nullptr, io, bo, U, 10, 8), MINER_EINVAL);
    EXPECT(advance(fb, ib, nullptr, ib, 100, ib, ib, ib, 8, fo, io, io, io, nullptr, bo, U, 10, 8), MINER_EINVAL);
    EXPECT(advance(fb, ib, nullptr, ib, 100, ib, ib, ib, 8, fo, io, io, io, io, nullptr, U, 10, 8), MINER_EINVAL);
    EXPECT(advance(fb, ib, nullptr, nullptr, 100, ib, ib, ib, 8, fo, io, io, io, io, bo, U, 10, 8), MINER_EINVAL);   // no group source
    EXPECT(advance(fb, ib, nullptr, ib, 0, ib, ib, ib, 8, fo, io, io, io, io, bo, U, 10, 8), MINER_EINVAL);
    EXPECT(advance(fodd, ib, nullptr, nullptr, 0, ib, ib, ib, 8, fo, io, io, io, io, bo, U, 10, 8), MINER_EINVAL);   // before the alignment
    EXPECT(advance(fodd, ib, nullptr, ib, 100, ib, ib, ib, 8, fo, io, io, io, io, bo, U, 10, 8), MINER_EALIGN);
    EXPECT(advance(fb, iodd, nullptr, ib, 100, ib, ib, ib, 8, fo, io, io, io, io, bo, U, 10, 8), MINER_EALIGN);
    EXPECT(advance(fb, ib, iodd, nullptr, 0, ib, ib, ib, 8, fo, io, io, io, io, bo, U, 10, 8), MINER_EALIGN);
    EXPECT(advance(fb, ib, nullptr, iodd, 100, ib, ib, ib, 8, fo, io, io, io, io, bo, U, 10, 8), MINER_EALIGN);
    EXPECT(advance(fb, ib, nullptr, ib, 100, iodd, ib, ib, 8, fo, io, io, io, io, bo, U, 10, 8), MINER_EALIGN);
    EXPECT(advance(fb, ib, nullptr, ib, 100, ib, iodd, ib, 8, fo, io, io, io, io, bo, U, 10, 8), MINER_EALIGN);
    EXPECT(advance(fb, ib, nullptr, ib, 100, ib, ib, iodd, 8, fo, io, io, io, io, bo, U, 10, 8), MINER_EALIGN);
    EXPECT(advance(fb, ib, nullptr, ib, 100, ib, ib, ib, 8, (float*)iood, io, io, io, io, bo, U, 10, 8), MINER_EALIGN);
    EXPECT(advance(fb, ib, nullptr, ib, 100, ib, ib, ib, 8, fo, iood, io, io, io, bo, U, 10, 8), MINER_EALIGN);
    EXPECT(advance(fb, ib, nullptr, ib, 100, ib, ib, ib, 8, fo, io, iood, io, io, bo, U, 10, 8), MINER_EALIGN);
    EXPECT(advance(fb, ib, nullptr, ib, 100, ib, ib, ib, 8, fo, io, io, iood, io, bo, U, 10, 8), MINER_EALIGN);
    EXPECT(advance(fb, ib, nullptr, ib, 100, ib, ib, ib, 8, fo, io, io, io, iood, bo, U, 10, 8), MINER_EALIGN);
  }
  // accepted: U == 0 returns after the validation
  EXPECT(advance(fb, ib, nullptr, ib, 100, ib, ib, ib, 8, fo, io, io, io, io, bo, 0, 10, 8), MINER_OK);
  EXPECT(advance(fb, ib, ib, nullptr, 0, ib, ib, ib, 8, fo, io, io, io, io, bo, 0, 10, 8), MINER_OK);           // groups given
  EXPECT(advance(fb, ib, ib, ib, 100, ib, ib, ib, 8, fo, io, io, io, io, bo + 1, 0, 256, QM), MINER_OK);        // both; a byte-aligned flag
  EXPECT(advance(fb, ib, ib, nullptr, 0, nullptr, nullptr, ib, 0, fo, io, nullptr, nullptr, io, bo, 0, 1, 0), MINER_OK);   // empty tables
  EXPECT(advance(fb, ib, ib, nullptr, 0, imis, imis, imis, QM, fo, io, io, io, io, bo, 0, 10, 8), MINER_OK);

  printf("abi_errors_resume: %d calls, %d failures\n", g_calls, g_fail);
  return g_fail ? 1 : 0;
}
