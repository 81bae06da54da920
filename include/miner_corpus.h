/*
 * miner_corpus.h — C ABI of the full-corpus ranking path of libminer_hip.so (MI355X, gfx950):
 * BASELINE config 5 ("1M users x 200k news, history=200, K=64, d=768, fp16"), SURVEY.md §7 step 6
 * and §8(d): every user against every news item of a table with the MINER click score, and a fused
 * top-k — the U x N score matrix is never materialised.
 *
 * The arithmetic is the reference's (MrRobot2211/miner, src/model/model.py), with the candidate set
 * of an impression replaced by the whole news table:
 *
 *   miner_encode_users(...)   per user: PolyAttention.forward (model.py:159-185) -> mui [K, d], and
 *                             for score_type 'weighted' the TargetAwareAttention projection
 *                             proj = gelu(mui · W2ᵀ) (model.py:212) [K, d].
 *   miner_rank_topk(...)      per (user, news n): M_k = mui_k · e_n (model.py:127) and
 *                             weighted: Σ_k softmax_k(proj_k · e_n) · M_k (model.py:213-214)
 *                             max / mean: max_k / mean_k M_k (model.py:128-131);
 *                             per user the topk best (score desc, news id asc on ties).
 *   miner_rank_topk_filtered(...)  the same, leaving out a per-user list of news ids (the clicked
 *                             history) and every news outside a table-wide eligibility bitmap.
 *   miner_rank_topk_subset(...)    the same over the table rows of an id list only (cost by the
 *                             list's length), and miner_topk_merge(...) to fold its lists into
 *                             lists ranked earlier: incremental ranking of a changing corpus.
 *   miner_score_pairs(...)    the click score of given (user, news) pairs, with the ranker's bits, and
 *   miner_rank_count(...)     per user and target (score, id), how many news rank before it: exact
 *                             full-corpus ranks, still without the U x N matrix.
 *   miner_rank_topk_biased(...), miner_score_pairs_biased(...), miner_rank_count_biased(...)
 *                             the ranking, pair and counting forms with a per-news fp32 prior added
 *                             to the click score before it is used.
 *   miner_rank_topk_capped(...), miner_topk_merge_capped(...)
 *                             the ranking and list-merge forms with at most `cap` news of one
 *                             cluster (story, publisher) per list.
 *   miner_rank_topk_after(...)     the ranking continued strictly after a (score, id) cursor per user.
 *   miner_score_pairs_interest(...), miner_rank_topk_interest(...), miner_topk_merge_grouped(...)
 *                             which of the user's K interests a news matched (the arg-max of the
 *                             score's own reduction over K), and lists with at most `interest_cap`
 *                             news of one dominant interest.
 *   miner_rank_topk_resume(...), miner_walk_advance(...)
 *                             a capped list continued on a later page: the cursor together with a
 *                             per-user table of how many entries of each group were already served,
 *                             and that state advanced by a served page on the device.
 *
 * Conventions are those of miner_score.h. dtype: MINER_DTYPE_F32 (exact fp32, parity mode),
 * MINER_DTYPE_BF16 or MINER_DTYPE_F16 (16-bit operands, fp32 accumulation and softmax).
 * Limits: L <= 256, K <= 64, Dc <= 256, d % 64 == 0 (fp32: d % 32 == 0), d <= 1024,
 * topk <= 256.
 */
#ifndef MINER_CORPUS_H
#define MINER_CORPUS_H

#include <stddef.h>
#include <stdint.h>

#include "miner_score.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MINER_CORPUS_MAX_L 256
#define MINER_CORPUS_MAX_K 64
#define MINER_CORPUS_MAX_TOPK 256

/* Weights of the user encoder (Dc and K up to 256 / 64), packed once per model:
 *   w_poly [Dc, d], context_codes [K, Dc], w_target [d, d] (NULL: no projection), all dtype. */
size_t miner_encoder_packed_bytes(int dtype, int d, int Dc, int K);
int miner_encoder_pack(void* stream, int dtype, const void* w_poly, const void* context_codes,
                       const void* w_target, int d, int Dc, int K, void* packed);

/*
 * Encode U users.
 *   history    [U, L, d] dtype (his_ids NULL), or the news table [n_news, d] with
 *   his_ids    [U, L] int32 rows of it (gather mode; clamped to [0, n_news) on the device)
 *   his_mask   [U, L] uint8, his_bias [U, L] fp32 or NULL (added to the logits, model.py:176)
 *   mui_f32    [U, K, d] fp32 out or NULL;  user_mui [U, K, d] dtype out (ranking operand);
 *   user_proj  [U, K, d] dtype out, gelu(mui · W2ᵀ), or NULL (the pack must hold w_target).
 */
int miner_encode_users(void* stream, int dtype, const void* history, const int32_t* his_ids, int n_news,
                       const uint8_t* his_mask, const float* his_bias, const void* packed, int U, int L,
                       int d, int Dc, int K, float* mui_f32, void* user_mui, void* user_proj);

/*
 * Rank every news item of `news` [N, d] for each of U users; top_scores [U, topk] fp32 and
 * top_ids [U, topk] int32, best first (rows past N: -inf / -1). score_type as miner_score.h
 * (WEIGHTED needs user_proj).
 */
int miner_rank_topk(void* stream, int dtype, int score_type, const void* user_mui, const void* user_proj,
                    const void* news, int U, int N, int d, int K, int topk, float* top_scores,
                    int32_t* top_ids);

/*
 * The same with a caller-owned device workspace of workspace_bytes bytes (16-byte aligned; NULL: the
 * form above). With a workspace of at least miner_rank_topk_workspace_bytes(U, topk) bytes, on a
 * 256-CU device, the split form runs: the news table is split in 8 slices whose per-user top-k
 * lists are merged by a second launch (8x the workgroups for small user batches), the users mapped
 * so that the CUs of one XCD share 8 users' rows in their L2. A smaller workspace is never written
 * (the unsplit form runs). Same results as miner_rank_topk, bit for bit.
 * miner_rank_topk_workspace_bytes returns 0 where the split form cannot run (not a 256-CU device,
 * invalid arguments). miner_rank_topk_split_recommended(U) is 1 where the split form is the faster
 * one (fewer than 256 two-user tiles: U <= 510), so a caller passes a workspace only then.
 */
size_t miner_rank_topk_workspace_bytes(int U, int topk);
int miner_rank_topk_split_recommended(int U);
int miner_rank_topk_ws(void* stream, int dtype, int score_type, const void* user_mui, const void* user_proj,
                       const void* news, int U, int N, int d, int K, int topk, float* top_scores,
                       int32_t* top_ids, void* workspace, size_t workspace_bytes);

/*
 * miner_rank_topk_ws with two optional filters on what a user's list may hold (the two calls above
 * are this one with both NULL). They decide only which (score, id) pairs are kept, inside the
 * ranker's threshold test; no score changes, and a list with fewer than topk survivors ends in
 * -inf / -1 entries. Split and unsplit forms agree bit for bit under the filters too.
 *   exclude_ids [U, E] int32, row-major, 0 <= E <= MINER_CORPUS_MAX_L: news ids that must not
 *               appear in user u's list (its clicked history, say). Entries outside [0, N) are
 *               ignored (-1 is the usual padding); duplicates are allowed. E == 0: no exclusion,
 *               whatever the pointer.
 *   news_ok     ceil(N / 32) uint32 words, or NULL for "every news": news n may be ranked iff
 *               bit (n & 31) of word (n >> 5) is set (bit 0 is the least significant). Bits at
 *               or past N in the last word are never read.
 * Both are device pointers, 4-byte aligned. Beyond miner_rank_topk_ws's checks: E < 0, or E > 0
 * with a NULL exclude_ids: MINER_EINVAL; E > MINER_CORPUS_MAX_L: MINER_ESHAPE; a misaligned
 * filter pointer: MINER_EALIGN (all before any launch).
 */
int miner_rank_topk_filtered(void* stream, int dtype, int score_type, const void* user_mui,
                             const void* user_proj, const void* news, int U, int N, int d, int K, int topk,
                             const int32_t* exclude_ids, int E, const uint32_t* news_ok,
                             float* top_scores, int32_t* top_ids, void* workspace, size_t workspace_bytes);

/*
 * miner_rank_topk_filtered over a subset of the table given as an id list: only the rows
 * news[news_ids[0 .. M)] are fetched and multiplied, so the cost follows M, not N (the bitmap form
 * streams all N rows whatever the bitmap holds).
 *   news_ids    [M] int32 device pointer, 4-byte aligned: distinct table rows, in any order (the
 *               list does not depend on it; ascending ids gather neighbouring rows together).
 *               Distinctness is a precondition: a repeated id may appear twice in a list. Ids
 *               outside [0, N) are never ranked and no row is read for them.
 * The result equals miner_rank_topk_filtered's on the same inputs with news_ok replaced by
 * news_ok AND "n is in news_ids" — scores and ids bit for bit, split and unsplit forms, every dtype
 * and score type; ids are table ids, ties rank the lower id first. exclude_ids and news_ok (either
 * may be NULL) apply to the table id. M == 0 writes (-inf, -1) everywhere without a ranker launch.
 * After miner_rank_topk_filtered's checks, in its order and with its codes: M < 0, or M > 0 with a
 * NULL news_ids: MINER_EINVAL; a misaligned news_ids: MINER_EALIGN (all before any launch).
 */
int miner_rank_topk_subset(void* stream, int dtype, int score_type, const void* user_mui,
                           const void* user_proj, const void* news, int U, int N, int d, int K, int topk,
                           const int32_t* exclude_ids, int E, const uint32_t* news_ok,
                           const int32_t* news_ids, int M, float* top_scores, int32_t* top_ids,
                           void* workspace, size_t workspace_bytes);

/*
 * Merge two per-user lists under the ranker's total order (score desc, news id asc):
 *   a_scores / a_ids [U, ka], b_scores / b_ids [U, kb], 0 <= ka, kb <= MINER_CORPUS_MAX_TOPK, each
 *   row a set of (score, id) pairs in any order, an entry with id < 0 (the (-inf, -1) tail of a
 *   ranked list) holding nothing; within one row the valid ids are distinct.
 *   out_scores / out_ids [U, topk], topk <= MINER_CORPUS_MAX_TOPK, distinct from the inputs: the
 *   best topk entries of the union, best first, then (-inf, -1). An id in both rows keeps b's
 *   entry (a fresh score replaces a stale one).
 *   news_ok     NULL, or the eligibility bitmap of miner_rank_topk_filtered over N news: entries
 *               whose bit is clear, or whose id is at or past N, drop out (N is read only then).
 * With miner_rank_topk_subset this is the incremental update: rank the fresh ids, merge the lists
 * into the served ones — for disjoint id sets the result is the list of ranking their union, bit for
 * bit. Device pointers, 4-byte aligned. Negative U / ka / kb, topk <= 0, a NULL pointer where
 * entries are expected, a bitmap with N <= 0: MINER_EINVAL; ka, kb or topk past the cap:
 * MINER_ESHAPE; a misaligned pointer: MINER_EALIGN (all before any launch).
 */
int miner_topk_merge(void* stream, const float* a_scores, const int32_t* a_ids, int ka, const float* b_scores,
                     const int32_t* b_ids, int kb, int U, int topk, const uint32_t* news_ok, int N,
                     float* out_scores, int32_t* out_ids);

/*
 * The click score of chosen (user, news) pairs from cached user vectors: the second stage of a
 * recommender (re-score a short candidate list per user), and the refresh of a served list.
 *   scores[u, c] = click score of (user u, news[cand_ids[u, c]]), bit for bit the score the ranking
 *   forms compute for that pair (every dtype, score type, K, d: the same d-chunk sequence, in-lane K
 *   reductions and lane-half exchanges, with the chunk count and K compile-time where the ranking
 *   forms have them).
 *   cand_ids    [U, C] int32 device pointer, 4-byte aligned, C >= 0, any order, repeats allowed; an
 *               id outside [0, N) gives -inf and no row is read for it.
 *   scores      [U, C] fp32 out, 4-byte aligned.
 * Only the U x C rows are fetched and multiplied (a workgroup takes one user and 256 entries of its
 * list per step). After the checks shared with miner_rank_topk_filtered (dtype, d, K, score_type,
 * U, N, the user and table pointers and their alignment), in its order and with its codes: C < 0,
 * or C > 0 with a NULL cand_ids or scores: MINER_EINVAL; a misaligned cand_ids or scores:
 * MINER_EALIGN (all before any launch). U == 0 or C == 0: MINER_OK with no launch.
 */
int miner_score_pairs(void* stream, int dtype, int score_type, const void* user_mui, const void* user_proj,
                      const void* news, int U, int N, int d, int K, const int32_t* cand_ids, int C, float* scores);

#define MINER_CORPUS_MAX_TARGETS 64

/*
 * The counting form of the ranker: exact full-corpus ranks without a list.
 *   counts[u, j] = #{ n in [0, N) : news_ok(n) and (score(u, n), n) ranks before
 *                    (target_scores[u, j], target_ids[u, j]) in the ranker's total order
 *                    (score desc, id asc) }.
 *   target_scores [U, T] fp32, target_ids [U, T] int32, 1 <= T <= MINER_CORPUS_MAX_TARGETS;
 *   news_ok     as in miner_rank_topk_filtered (NULL: every news); counts [U, T] int32 out.
 * With target_scores from miner_score_pairs on target_ids, counts[u, j] is the 0-based rank of the
 * target among the eligible news: the stream's score of the target's own row equals the given one
 * bit for bit, so the target does not count itself, and ties rank by id. A news whose score is NaN
 * is never counted; a NaN target score counts nothing. The table is streamed once for all T
 * targets; there is no per-user exclusion list (subtract the excluded ids that rank before the
 * target, scored with miner_score_pairs — corpus.rank_of does). One launch, the unsplit form: no
 * workspace, no atomics, a deterministic result.
 * All pointers are device pointers, 4-byte aligned. After the shared checks (above): T <= 0, or a
 * NULL target_scores / target_ids / counts: MINER_EINVAL; T > MINER_CORPUS_MAX_TARGETS:
 * MINER_ESHAPE; a misaligned pointer: MINER_EALIGN (all before any launch). U == 0: MINER_OK.
 */
int miner_rank_count(void* stream, int dtype, int score_type, const void* user_mui, const void* user_proj,
                     const void* news, int U, int N, int d, int K, const float* target_scores,
                     const int32_t* target_ids, int T, const uint32_t* news_ok, int32_t* counts);

/*
 * Score priors applied at rank time: the three forms above with a per-news fp32 prior added to the
 * click score (recency decay, popularity, an editorial boost, a per-edition weight — whatever the
 * feed adds before it ranks; the table may change between any two calls).
 *   news_bias   [G, N] fp32, row-major, G >= 1: the prior of news n for the users of group g at
 *               news_bias[g * N + n].
 *   user_group  [U] int32, user u's row of news_bias, or NULL for "row 0 for every user". A value
 *               outside [0, G) is the caller's error; the device clamps it into [0, G), so no
 *               address leaves the table, and the result is then that of the clamped row.
 * For user u and table row n every form uses
 *   biased(u, n) = fp32_add_rn(score(u, n), news_bias[group(u)][n])
 * where score(u, n) is exactly the fp32 value the unbiased form computes and the add is one separate
 * IEEE addition (never contracted into the divide before it), so "scores + prior" in fp32 on any
 * IEEE machine reproduces it bit for bit. The biased value is what is compared, listed, returned,
 * counted against and stored; everything else — ties by the lower id, exclusion lists, the bitmap,
 * subset ids, (-inf, -1) past N, -inf for a pair id outside [0, N) (no prior is read for it) —
 * applies to the table id as before. A prior is not a filter: a -inf prior still lists the news
 * while a list is not full (use news_ok to remove it); a +inf prior ranks it first (ties among
 * them by id); a NaN sum is never listed or counted. Split and unsplit forms agree bit for bit.
 *
 * miner_rank_topk_biased: miner_rank_topk_subset's arguments, then the three above. news_ids NULL
 * with M < 0 selects the whole table (miner_rank_topk_filtered); otherwise the subset rules hold.
 * miner_score_pairs_biased / miner_rank_count_biased: miner_score_pairs / miner_rank_count plus the
 * three; target_scores are biased scores (miner_score_pairs_biased's, for exact ranks).
 * With news_bias NULL (and user_group NULL) each returns exactly what the unbiased call returns: it
 * launches the same kernel. After the unbiased call's own argument checks, in their order and with
 * their codes: news_bias non-NULL with G <= 0, or news_bias NULL with a non-NULL user_group:
 * MINER_EINVAL; a news_bias, then a user_group, that is not 4-byte aligned: MINER_EALIGN (all
 * before any launch, and before the U == 0 / C == 0 returns).
 */
int miner_rank_topk_biased(void* stream, int dtype, int score_type, const void* user_mui,
                           const void* user_proj, const void* news, int U, int N, int d, int K, int topk,
                           const int32_t* exclude_ids, int E, const uint32_t* news_ok,
                           const int32_t* news_ids, int M, float* top_scores, int32_t* top_ids,
                           void* workspace, size_t workspace_bytes, const float* news_bias, int G,
                           const int32_t* user_group);
int miner_score_pairs_biased(void* stream, int dtype, int score_type, const void* user_mui,
                             const void* user_proj, const void* news, int U, int N, int d, int K,
                             const int32_t* cand_ids, int C, float* scores, const float* news_bias, int G,
                             const int32_t* user_group);
int miner_rank_count_biased(void* stream, int dtype, int score_type, const void* user_mui,
                            const void* user_proj, const void* news, int U, int N, int d, int K,
                            const float* target_scores, const int32_t* target_ids, int T,
                            const uint32_t* news_ok, int32_t* counts, const float* news_bias, int G,
                            const int32_t* user_group);

/*
 * Per-cluster caps: at most `cap` news of one cluster (a story, a publisher, a sub-category) in a
 * user's list.
 *   news_cluster [N] int32 device pointer, 4-byte aligned: news_cluster[n] >= 0 is the cluster of
 *               news n (arbitrary non-negative values, need not be dense); < 0: in no cluster, never
 *               capped.
 *   cap         1 <= cap <= MINER_CORPUS_MAX_TOPK, one value for every cluster and user.
 * User u's capped list is a walk of its complete ranking — the one the uncapped call would give with
 * topk = N under the same exclude_ids, news_ok, news_ids and news_bias, score descending, then lower
 * news id: an entry is kept iff fewer than cap entries of its cluster were kept before it (an
 * unclustered entry always); the walk stops after topk kept entries, and a shorter list ends in
 * (-inf, -1). No score changes: a listed entry carries, bit for bit, the score the uncapped call
 * gives that pair. An excluded or ineligible news does not use up its cluster's cap; a NaN score is
 * never listed and does not count. Within a cluster the best cap survivors are kept, so capped lists
 * merge as top-k lists do: capped(A u B) = capped(capped(A) u capped(B)) for disjoint A and B.
 *
 * miner_rank_topk_capped: miner_rank_topk_biased's arguments (news_ids NULL with M < 0: the whole
 * table; news_bias / user_group present or NULL), then the two above. Every dtype, score type, K and
 * d of the biased form. With news_cluster NULL it returns exactly what miner_rank_topk_biased returns
 * on the other arguments (it launches the same kernel; cap is read only with a table, as G is).
 * With a table the UNSPLIT form runs whatever the workspace: a workspace is accepted (checked as
 * before) and never written — there is no split form under caps, so a small batch (U <= 510) does
 * not get the split form's 8x workgroups.
 *
 * miner_topk_merge_capped: miner_topk_merge (b-over-a replacement, then the bitmap pruning), then the
 * best topk of the capped walk over what is left. The input rows need not be sorted and need not be
 * capped themselves (an uncapped list through this call with ka = 0 is its post-hoc cap: the first
 * entries of the true capped list, and all of it wherever it fills topk or the input was not full).
 *   news_cluster holds n_cluster entries; an entry whose id is at or past n_cluster is in no
 *   cluster and no table word is read for it. With news_cluster NULL it is miner_topk_merge.
 * After the base call's own checks, in their order and with their codes: a table with cap <= 0:
 * MINER_EINVAL; cap > MINER_CORPUS_MAX_TOPK: MINER_ESHAPE; (merge form) a table with
 * n_cluster <= 0: MINER_EINVAL; a misaligned news_cluster: MINER_EALIGN (all before any launch, and
 * before the U == 0 return).
 */
int miner_rank_topk_capped(void* stream, int dtype, int score_type, const void* user_mui,
                           const void* user_proj, const void* news, int U, int N, int d, int K, int topk,
                           const int32_t* exclude_ids, int E, const uint32_t* news_ok,
                           const int32_t* news_ids, int M, float* top_scores, int32_t* top_ids,
                           void* workspace, size_t workspace_bytes, const float* news_bias, int G,
                           const int32_t* user_group, const int32_t* news_cluster, int cap);
int miner_topk_merge_capped(void* stream, const float* a_scores, const int32_t* a_ids, int ka,
                            const float* b_scores, const int32_t* b_ids, int kb, int U, int topk,
                            const uint32_t* news_ok, int N, float* out_scores, int32_t* out_ids,
                            const int32_t* news_cluster, int n_cluster, int cap);

/*
 * Keyset cursors: a user's ranking continued after a given entry, for lists of any depth as pages of
 * up to MINER_CORPUS_MAX_TOPK entries that each stream the table once.
 *   after_scores [U] fp32, after_ids [U] int32, device pointers, 4-byte aligned, both or neither.
 * The ranking order is the ranker's strict total order: score descending, then lower news id, where
 * the score is the value that is ranked (the biased sum under news_bias) and the id the table id
 * (also in the subset form). User u's list holds the first topk entries of its ranking — under the
 * same exclude_ids, news_ok, news_ids and news_bias — that come STRICTLY AFTER the pair
 * (after_scores[u], after_ids[u]): score < after_scores[u], or score == after_scores[u] (a float
 * compare: -0 equals +0) and id > after_ids[u]; then (-inf, -1). A listed entry carries, bit for bit,
 * the score of the call without a cursor. Passing each row's last entry back continues the ranking
 * where that row ended; the pages of a user are disjoint and concatenate to its complete ranking.
 *   (+inf, -1)        "before everything": every listable entry comes after it (the first page).
 *   (-inf, 2^31 - 1)  "after everything": nothing comes after it. NOT the (-inf, -1) tail of a short
 *                     row: a cursor there would list the news that score -inf once more.
 *   a NaN score       lists nothing.
 * The cursor need not be a listed news: an id that is excluded, ineligible, outside news_ids,
 * negative or past N is a position in the order like any other. Split and unsplit forms agree bit
 * for bit (every slice applies the cursor). A cursor alone does not continue a capped list: a capped
 * walk also needs the per-cluster counts of the earlier pages, which a (score, id) pair does not
 * carry — this entry refuses the pair, and miner_rank_topk_resume (below) takes those counts.
 *
 * miner_rank_topk_after: miner_rank_topk_capped's arguments, then the two above. With both NULL it
 * returns exactly what miner_rank_topk_capped returns on the other arguments (it launches the same
 * kernel). With a cursor the cursor form of the ranker runs, over the table or the id list, split or
 * unsplit, with any of exclude_ids, news_ok and news_bias NULL or not; a call without a cursor
 * launches no code of it. After the capped call's own checks, in their order and with
 * their codes: one of after_scores / after_ids NULL and the other not: MINER_EINVAL; a cursor with
 * a non-NULL news_cluster: MINER_EINVAL; a misaligned after_scores or after_ids: MINER_EALIGN (all
 * before any launch, and before the U == 0 return).
 */
int miner_rank_topk_after(void* stream, int dtype, int score_type, const void* user_mui,
                          const void* user_proj, const void* news, int U, int N, int d, int K, int topk,
                          const int32_t* exclude_ids, int E, const uint32_t* news_ok,
                          const int32_t* news_ids, int M, float* top_scores, int32_t* top_ids,
                          void* workspace, size_t workspace_bytes, const float* news_bias, int G,
                          const int32_t* user_group, const int32_t* news_cluster, int cap,
                          const float* after_scores, const int32_t* after_ids);

/*
 * The dominant interest of a pair, and per-interest caps: what MINER's K interest vectors add to a
 * served list — which of the user's interests a news matched, and lists that cover several of them.
 *   interest(u, n) = the lowest k in [0, K) whose value equals the maximum the score's own reduction
 *   over K found: for MINER_SCORE_WEIGHTED over the logits proj_k · e_n (the largest target-aware
 *   softmax weight, model.py:213), for MINER_SCORE_MAX over M_k = mui_k · e_n (model.py:129). It is
 *   read off the very accumulators the score is made from, after the contraction, so no score bit
 *   changes; ties go to the lowest k; if no k compares equal (every value NaN) it is -1, "in no
 *   group". A prior (news_bias) does not enter it. MINER_SCORE_MEAN has no dominant interest: asking
 *   for one is MINER_EINVAL.
 *
 * miner_score_pairs_interest: miner_score_pairs_biased's arguments, then
 *   interests   [U, C] int32 out, device pointer, 4-byte aligned: interest(u, cand_ids[u, c]) next to
 *               scores[u, c]; -1 for an id outside [0, N).
 * scores are, bit for bit, miner_score_pairs_biased's. With interests NULL it returns exactly what
 * miner_score_pairs_biased returns: it launches the same kernel. After that call's own checks, in
 * their order and with their codes: interests with MINER_SCORE_MEAN: MINER_EINVAL; a misaligned
 * interests: MINER_EALIGN (all before any launch, and before the U == 0 / C == 0 returns).
 *
 * miner_rank_topk_interest: miner_rank_topk_after's arguments, then
 *   interest_cap  0: none — with top_interest NULL the call returns exactly what
 *               miner_rank_topk_after returns on the other arguments (it launches the same kernel);
 *               1 <= interest_cap <= MINER_CORPUS_MAX_TOPK: at most interest_cap news of one
 *               dominant interest in a user's list.
 *   top_interest  [U, topk] int32 out or NULL (only under a cap), 4-byte aligned: interest(u, .) of
 *               the listed entries, -1 in the (-inf, -1) tail.
 * User u's list is the walk of its complete ranking — under exclude_ids, news_ok, news_ids and
 * news_bias, as the uncapped call gives it with topk = N — that keeps an entry iff fewer than
 * interest_cap kept entries before it have the same interest(u, .); an entry with interest -1 is
 * always kept; the walk stops after topk kept entries, then (-inf, -1). A listed score is the uncapped
 * call's, bit for bit. This is exactly miner_rank_topk_capped for that one user with the cluster
 * table g_u[n] = interest(u, n) (news_cluster cannot express it for more than one user: its cluster
 * belongs to the news, the dominant interest to the pair). As the capped form: the UNSPLIT kernel
 * whatever the workspace (accepted, never written), over the table or the id list, with or without
 * a prior; no bare cursor (miner_rank_topk_resume continues it), and never together with news_cluster. After miner_rank_topk_after's own
 * checks, in their order and with their codes: interest_cap < 0: MINER_EINVAL;
 * interest_cap > MINER_CORPUS_MAX_TOPK: MINER_ESHAPE; a cap with a non-NULL news_cluster or with a
 * cursor: MINER_EINVAL; a cap with MINER_SCORE_MEAN: MINER_EINVAL; top_interest without a cap:
 * MINER_EINVAL; a misaligned top_interest: MINER_EALIGN (all before any launch, and before the
 * U == 0 return).
 *
 * miner_topk_merge_grouped: miner_topk_merge's arguments, then per-entry groups and a cap —
 *   a_groups [U, ka], b_groups [U, kb] int32: the group of each entry (its interest; < 0: none),
 *   out_groups [U, topk] int32 out: the groups of the merged entries, -1 in the tail,
 *   cap         0: the groups are only carried; 1 <= cap <= MINER_CORPUS_MAX_TOPK: after the
 *               replacement and the pruning, the capped walk of miner_topk_merge_capped over what is
 *               left, with an entry's own group in place of news_cluster[id].
 * An id in both rows keeps b's entry and b's group. With cap == 0 out_scores / out_ids are
 * miner_topk_merge's, bit for bit. Interest-capped lists of one user merge as capped lists do:
 * for disjoint id sets the result is the interest-capped ranking of their union, bit for bit. After
 * miner_topk_merge's own checks, in their order and with their codes: cap < 0: MINER_EINVAL;
 * cap > MINER_CORPUS_MAX_TOPK: MINER_ESHAPE; a NULL a_groups with ka > 0, b_groups with kb > 0, or
 * out_groups: MINER_EINVAL; a misaligned group pointer: MINER_EALIGN (all before any launch, and
 * before the U == 0 return).
 */
int miner_score_pairs_interest(void* stream, int dtype, int score_type, const void* user_mui,
                               const void* user_proj, const void* news, int U, int N, int d, int K,
                               const int32_t* cand_ids, int C, float* scores, const float* news_bias, int G,
                               const int32_t* user_group, int32_t* interests);
int miner_rank_topk_interest(void* stream, int dtype, int score_type, const void* user_mui,
                             const void* user_proj, const void* news, int U, int N, int d, int K, int topk,
                             const int32_t* exclude_ids, int E, const uint32_t* news_ok,
                             const int32_t* news_ids, int M, float* top_scores, int32_t* top_ids,
                             void* workspace, size_t workspace_bytes, const float* news_bias, int G,
                             const int32_t* user_group, const int32_t* news_cluster, int cap,
                             const float* after_scores, const int32_t* after_ids, int interest_cap,
                             int32_t* top_interest);
int miner_topk_merge_grouped(void* stream, const float* a_scores, const int32_t* a_ids, int ka,
                             const float* b_scores, const int32_t* b_ids, int kb, int U, int topk,
                             const uint32_t* news_ok, int N, float* out_scores, int32_t* out_ids,
                             const int32_t* a_groups, const int32_t* b_groups, int32_t* out_groups, int cap);

#define MINER_CORPUS_MAX_WALK_GROUPS 1024

/*
 * The resumed capped walk: a cursor under caps. A capped list (news_cluster / cap, or interest_cap)
 * continued on a later page needs, beside the (score, id) cursor, how many entries of each group the
 * earlier pages served. For user u the WALK STATE is
 *   a cursor (after_scores[u], after_ids[u]), and
 *   a table of n_used[u] pairs (used_groups[u][i], used_counts[u][i]), i < n_used[u], the groups
 *   STRICTLY ASCENDING and all >= 0 — a group is a cluster id under news_cluster, an interest in [0, K)
 *   under interest_cap. used(g) is the count of g's pair, 0 for a group not in the table; a negative
 *   count reads as 0.
 *   used_groups / used_counts [U, Q] int32 row-major, n_used [U] int32, device pointers, 4-byte
 *   aligned, 0 <= Q <= MINER_CORPUS_MAX_WALK_GROUPS. Only the first n_used[u] pairs of a row are read.
 *   Sortedness is a precondition, as the distinctness of news_ids is: over an unsorted table the
 *   lookup may miss a pair (its group then counts from 0). n_used[u] outside [0, Q] is the caller's
 *   error; the device clamps it into [0, Q], so no address leaves the table. The tables are only read.
 * The resumed list is the walk of u's complete ranking — under exclude_ids, news_ok, news_ids and
 * news_bias, score descending, then lower id — over the entries STRICTLY AFTER the cursor
 * (miner_rank_topk_after's rule, on the ranked value and the table id): an entry is kept iff its
 * group is negative or used(g) + (entries of g kept earlier in this call) < cap; the walk stops after
 * topk kept entries, then (-inf, -1). Listed scores are the uncapped call's, bit for bit; an excluded
 * or ineligible news spends no cap; a NaN score is never listed and a NaN cursor lists nothing. So
 * the pages chained through the state — the next state is the page's cursor (page_cursor's rule)
 * plus the old counts plus the groups of the page's kept entries: miner_walk_advance — concatenate to
 * the capped walk of any depth, also when cap or topk change between pages (both are read per call).
 * An empty table at (+inf, -1) gives miner_rank_topk_interest's capped list, bit for bit.
 * As the capped form: the UNSPLIT kernel whatever the workspace, over the table or the id list, with
 * or without a prior; one kind of cap per call; not for MINER_SCORE_MEAN with interests.
 *
 * miner_rank_topk_resume: miner_rank_topk_interest's arguments, then the three tables and Q. With
 * all three NULL it returns exactly what miner_rank_topk_interest returns (it launches the same
 * kernel; a cursor under caps is still MINER_EINVAL; Q is not read). With a table: that call's own
 * checks first, in their order and with their codes, except its refusal of a cursor under a cap; then
 * no cursor: MINER_EINVAL; neither kind of cap: MINER_EINVAL; Q < 0 or a NULL among the three:
 * MINER_EINVAL; Q > MINER_CORPUS_MAX_WALK_GROUPS: MINER_ESHAPE; a misaligned table pointer:
 * MINER_EALIGN (all before any launch, and before the U == 0 return).
 *
 * miner_walk_advance: the state after a served page, on the device (one small launch; a feed loop or
 * a deep list needs no host synchronisation).
 *   page_scores / page_ids [U, k], 1 <= k <= MINER_CORPUS_MAX_TOPK: the page as the ranker returned it.
 *   page_groups [U, k] int32 or NULL: the group of each entry (the interests listed with it); NULL:
 *               the group is news_cluster[id] (n_cluster entries; an id at or past n_cluster has no
 *               group and no word is read for it). An entry with id < 0 (the tail) or a negative group
 *               adds nothing.
 *   in_groups / in_counts [U, Q_in], in_n_used [U]: the state's table (as above; n clamped).
 *   out_after_scores / out_after_ids [U]: the row's last entry if the row is full, else
 *               (-inf, 2^31 - 1) — "after everything": the ranking ended.
 *   out_groups / out_counts [U, Q], out_n_used [U]: the union, strictly ascending, counts summed
 *               (a negative in count as 0). Distinct from the in buffers.
 *   overflow    [U] uint8 out: 1 if user u needs more than Q distinct groups — then its cursor
 *               becomes (-inf, 2^31 - 1), so its ranking ends rather than ever breaking a cap (the Q
 *               lowest groups are written); else 0.
 * U < 0, k <= 0, Q < 0 or Q_in < 0: MINER_EINVAL; k > MINER_CORPUS_MAX_TOPK, Q or Q_in >
 * MINER_CORPUS_MAX_WALK_GROUPS: MINER_ESHAPE; a NULL page, in_n_used or output pointer, NULL in
 * tables with Q_in > 0, NULL out tables with Q > 0: MINER_EINVAL; neither page_groups nor a
 * news_cluster with n_cluster > 0: MINER_EINVAL; a misaligned pointer: MINER_EALIGN (all before any
 * launch, and before the U == 0 return).
 */
int miner_rank_topk_resume(void* stream, int dtype, int score_type, const void* user_mui,
                           const void* user_proj, const void* news, int U, int N, int d, int K, int topk,
                           const int32_t* exclude_ids, int E, const uint32_t* news_ok,
                           const int32_t* news_ids, int M, float* top_scores, int32_t* top_ids,
                           void* workspace, size_t workspace_bytes, const float* news_bias, int G,
                           const int32_t* user_group, const int32_t* news_cluster, int cap,
                           const float* after_scores, const int32_t* after_ids, int interest_cap,
                           int32_t* top_interest, const int32_t* used_groups, const int32_t* used_counts,
                           const int32_t* n_used, int Q);
int miner_walk_advance(void* stream, const float* page_scores, const int32_t* page_ids,
                       const int32_t* page_groups, const int32_t* news_cluster, int n_cluster,
                       const int32_t* in_groups, const int32_t* in_counts, const int32_t* in_n_used, int Q_in,
                       float* out_after_scores, int32_t* out_after_ids, int32_t* out_groups,
                       int32_t* out_counts, int32_t* out_n_used, uint8_t* overflow, int U, int k, int Q);

#ifdef __cplusplus
}
#endif

#endif /* MINER_CORPUS_H */
