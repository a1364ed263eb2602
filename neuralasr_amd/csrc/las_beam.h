// las_beam.h — launch wrappers of the LAS beam search's kernels (las_beam.hip; internal, C++).  Layouts: las.h; beam rows
// r = b*W + k (utterance b, beam k), R rows launched, rows >= B*W padding.
#pragma once
#include "las.h"

namespace nasr {

// done: the search's "every beam finished" word, read first by every step kernel
// ctx: the rows' n-gram context indices (K = C^(order-1) contexts, ctx0 = start_id in every digit; K = 1 and 0 without a
// table); table [K][C] or nullptr: weight * table[ctx][w] joins an unfinished row's log-probs
void launch_las_beam_init(const float* out4, const float* c4, int L4, int Bp, int W, int nrows, int R, int start_id, float* S,
                          float* c, int32_t* ids, float* logp, int32_t* len, int32_t* fin, int32_t* ctx, int ctx0,
                          hipStream_t st);
void launch_las_beam_score(const float* logits, int Cp, int C, const float* logp, const int32_t* len, const int32_t* fin,
                           const float* pen, int end_id, int nrows, const float* table, const int32_t* ctx, float weight,
                           float* scores, float* totals, const int32_t* done, hipStream_t st);
void launch_las_beam_select(const float* scores, int B, int W, int C, int32_t* sel_idx, float* sel_score, const int32_t* done,
                            hipStream_t st);
void launch_las_beam_update(const int32_t* sel_idx, const float* sel_score, const float* totals, int W, int C, int end_id,
                            int nrows, const float* Sx, const float* cx, const int32_t* len_in, const int32_t* fin_in,
                            const int32_t* ctx_in, int K, float* S, float* c, int32_t* ids, float* logp_out, int32_t* len_out,
                            int32_t* fin_out, int32_t* ctx_out, float* tr_score, int32_t* tr_word, int32_t* tr_parent,
                            const int32_t* done, hipStream_t st);
// flags [2]: done, steps run
void launch_las_beam_finish(const int32_t* fin, int nrows, int t, int max_steps, int32_t* flags, hipStream_t st);
void launch_las_beam_gather_tree(const int32_t* word, const int32_t* parent, const int32_t* len, int Tdec, int B, int W,
                                 int end_id, int32_t* out, hipStream_t st);

}  // namespace nasr
