/*
 * miner_diversify.h — C ABI of the diversity re-ranking stage of libminer_hip.so (MI355X, gfx950):
 * maximal marginal relevance (MMR) over a ranked pool, on the device. Where news_cluster / cluster_cap
 * and interest_cap (miner_corpus.h) are hard rules over a table someone chose, this is the soft one: a
 * news item's click score traded against its cosine similarity, in the news table's own embedding
 * space, to what the page already holds. The reference project has no such stage; the definition
 * below is the contract (tests/diversify_ref.py restates it in float64).
 *
 * Per user the input is a pool of P <= MINER_DIVERSIFY_MAX_POOL entries (in_scores[u, p],
 * in_ids[u, p]), in the order given (position p) — a list of miner_rank_topk* / miner_topk_merge*, or
 * any rows of (score, id) pairs; `news` is the table [N, d] in dtype MINER_DTYPE_F16, _BF16 or _F32.
 *
 *   candidates  entry p is a candidate iff 0 <= id_p < N and score_p is finite. A non-candidate — the
 *               (-inf, -1) tail of a short list, an id outside the table, a NaN or infinite score — is
 *               never listed and no table row is read for it. Repeated ids are allowed: each position
 *               is its own candidate.
 *   relevance   MINER_DIVERSIFY_REL_SCORE:  rel_p = score_p.
 *               MINER_DIVERSIFY_REL_MINMAX: rel_p = (score_p - s_min) / (s_max - s_min) over the
 *               user's candidates, one fp32 subtract each and one IEEE divide; 0 where s_max == s_min.
 *   similarity  the cosine of the table rows e_p = news[id_p]: G_pq = e_p · e_q with the products
 *               accumulated in fp32 on the matrix cores (v_mfma_f32_32x32x16_f16 / _bf16, the fp32
 *               MFMA for fp32 tables), sim_pq = G_pq / (sqrtf(G_pp) * sqrtf(G_qq)) with a correctly
 *               rounded sqrt, product and divide; sim_pq = 0 where G_pp == 0, G_qq == 0 or the
 *               quotient is not finite (a row holding an inf or a NaN is similar to nothing).
 *   walk        S = {}; for t = 0 .. topk-1 pick the candidate p not in S with the largest
 *                 obj_p = lambda * rel_p - (1.0f - lambda) * m_p,   m_p = max over q in S of sim_pq
 *               (m_p = 0 while S is empty): two fp32 products and one fp32 subtract, never contracted
 *               into an fma; the compare is on that fp32 value (-0 equals +0), ties go to the lower
 *               position, and an obj that is NaN compares as -inf. p joins S. The walk stops when no
 *               candidate is left.
 *   outputs     [U, topk] each: out_scores the entry's input score (its bits untouched), out_ids,
 *               out_pos (int32, the position in the pool), out_obj (fp32, the objective at the moment
 *               of selection; NULL: not written). Past the walk's end a row holds (-inf, -1, -1),
 *               and -inf in out_obj.
 *
 * At lambda == 1 the result is the pool's candidates by rel, ties by position: for a ranked list its
 * own prefix. The result is a subset of the pool in another order, so a pool ranked under caps keeps
 * its caps; it is NOT in score order, so it is no input for miner_topk_merge*.
 * Every user is one workgroup and depends on no other: a batch gives, bit for bit, what its users
 * give alone. Scores whose range s_max - s_min overflows fp32 are outside the contract (no address
 * depends on them).
 *
 * All pointers are device pointers. Argument checks, all before any launch and in this order:
 *   1. a dtype other than the three above, or an unknown relevance:           MINER_EINVAL
 *   2. U < 0, N <= 0, P <= 0 or topk <= 0:                                    MINER_EINVAL
 *   3. a NULL news, in_scores, in_ids, out_scores, out_ids or out_pos:        MINER_EINVAL
 *   4. lambda outside [0, 1], or NaN:                                         MINER_EINVAL
 *   5. P > MINER_DIVERSIFY_MAX_POOL, topk > P, or a d the ranker does not take
 *      (d <= 0, d > 1024, d % 64 != 0, for fp32 d % 32 != 0):                 MINER_ESHAPE
 *   6. in_scores, in_ids, out_scores, out_ids, out_pos or out_obj not 4-byte
 *      aligned, or news not 16-byte aligned:                                  MINER_EALIGN
 *   7. U == 0:                                                                MINER_OK, no launch
 */
#ifndef MINER_DIVERSIFY_H
#define MINER_DIVERSIFY_H

#include <stddef.h>
#include <stdint.h>

#include "miner_score.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MINER_DIVERSIFY_MAX_POOL 256

enum {
  MINER_DIVERSIFY_REL_SCORE = 0,
  MINER_DIVERSIFY_REL_MINMAX = 1
};

int miner_topk_diversify(void* stream, int dtype, const void* news, int N, int d,
                         const float* in_scores, const int32_t* in_ids, int U, int P, int topk,
                         float lambda, int relevance,
                         float* out_scores, int32_t* out_ids, int32_t* out_pos, float* out_obj /* NULL ok */);

#ifdef __cplusplus
}
#endif

#endif /* MINER_DIVERSIFY_H */
