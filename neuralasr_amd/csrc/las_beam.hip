// las_beam.hip — the kernels of the LAS inference graph's beam search (tf.contrib.seq2seq.BeamSearchDecoder of TF 1.15,
// DESIGN.md §10): the tiled initial state, the step's scores, an exact per-utterance top-W, the state update by parent and
// gather_tree.  nasr_las.hip orchestrates; the decoder step itself (cell, attention of a beam row over its utterance's
// memory, every product) is the training path's (las.hip, gemm.hip), as are wave_sum and the final-state gather (las.h).
//
// Beam rows r = b*W + k (utterance b, beam k), R = rup(B*W, 16) rows; rows >= B*W are padding that no selection reads.
// Every kernel of a step after the one that finished every beam returns at once: *done (set by las_beam_finish) is read
// at the top, so the host enqueues steps without waiting and reads the word once per chunk of steps.
//
// n-gram fusion: every beam row carries the context index of its hypothesis (the last order-1 ids, the
// most recent as the lowest digit, K = C^(order-1) contexts; 0 and K = 1 without a table); the score kernel adds
// weight * table[ctx][w] to an unfinished row's log-probs, the update derives the row's next context from its parent's.
#include "las_beam.h"

#include <cfloat>
#include <cmath>

namespace nasr {

namespace {
__device__ __forceinline__ float wave_max_b(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
// order-preserving map of a float onto uint32 (larger float -> larger key), and back
__device__ __forceinline__ uint32_t ord_key(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord_val(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
// lp + weight * t as a rounded product and a rounded sum (no fused multiply-add: tests/las_beam_lm_ref.py follows it
// operation by operation)
__device__ __forceinline__ float lm_fuse(float lp, float weight, float t) {
#pragma clang fp contract(off)
  const float p = weight * t;
  return lp + p;
}
}  // namespace

// S [R][LAS_SW] = [a = 0 | h = (h_fw final; h_bw final) of utterance r / W], c [R][LAS_HD], ids = start_id, log_probs =
// (0, -inf, -inf, ...), finished = (0, 1, 1, ...), lengths = 0, ctx = ctx0 (start_id in every digit) (block r, 512 threads)
__global__ __launch_bounds__(512) void las_beam_init_kernel(const float* __restrict__ out4, const float* __restrict__ c4, int L4,
                                                            int Bp, int W, int nrows, int start_id, float* __restrict__ S,
                                                            float* __restrict__ c, int32_t* __restrict__ ids,
                                                            float* __restrict__ logp, int32_t* __restrict__ len,
                                                            int32_t* __restrict__ fin, int32_t* __restrict__ ctx, int ctx0) {
  const int r = blockIdx.x, k = threadIdx.x;
  las_final_state(out4, c4, L4, Bp, r / W, r < nrows, k, S + (size_t)r * LAS_SW, c + (size_t)r * LAS_HD);
  if (k == 0) {
    const int kb = r < nrows ? r % W : 1;
    ids[r] = start_id;
    logp[r] = kb == 0 ? 0.f : -INFINITY;
    len[r] = 0;
    fin[r] = kb != 0;
    ctx[r] = ctx0;
  }
}

void launch_las_beam_init(const float* out4, const float* c4, int L4, int Bp, int W, int nrows, int R, int start_id, float* S,
                          float* c, int32_t* ids, float* logp, int32_t* len, int32_t* fin, int32_t* ctx, int ctx0,
                          hipStream_t st) {
  hipLaunchKernelGGL(las_beam_init_kernel, dim3(R), dim3(LAS_HD), 0, st, out4, c4, L4, Bp, W, nrows, start_id, S, c, ids, logp,
                     len, fin, ctx, ctx0);
}

// One wave per beam row: lp = (l - max) - log(sum exp(l - max)) (the sum: lane-strided partials, then a fixed butterfly);
// a finished row's lp is 0 at end_id and FLT_LOWEST elsewhere; total = log_probs + lp; score = total / pen[len_s],
// len_s = lengths + (!finished && w != end_id).  scores / totals [B*W][C]: utterance b's flat candidate k*C + w.
// table != nullptr (the same for every wave of the launch): an unfinished row's lp gets weight * table[ctx[r]][w] added, the
// row's C contiguous floats of the [K][C] table read lane-strided like the logits.
__global__ __launch_bounds__(256) void las_beam_score_kernel(const float* __restrict__ logits, int Cp, int C,
                                                             const float* __restrict__ logp, const int32_t* __restrict__ len,
                                                             const int32_t* __restrict__ fin, const float* __restrict__ pen,
                                                             int end_id, int nrows, const float* __restrict__ table,
                                                             const int32_t* __restrict__ ctx, float weight,
                                                             float* __restrict__ scores, float* __restrict__ totals,
                                                             const int32_t* __restrict__ done) {
  if (*done) return;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= nrows) return;
  const float* l = logits + (size_t)r * Cp;
  float m = -INFINITY;
  for (int w = lane; w < C; w += 64) m = fmaxf(m, l[w]);
  m = wave_max_b(m);
  float z = 0.f;
  for (int w = lane; w < C; w += 64) z += expf(l[w] - m);
  z = wave_sum(z);
  const float lse = logf(z);
  const bool f = fin[r] != 0;
  const float lp0 = logp[r];
  const int n0 = len[r];
  const float* trow = (table && !f) ? table + (size_t)ctx[r] * C : nullptr;
  float* sc = scores + (size_t)r * C;
  float* to = totals + (size_t)r * C;
  for (int w = lane; w < C; w += 64) {
    float lp = f ? (w == end_id ? 0.f : -FLT_MAX) : (l[w] - m) - lse;
    if (trow) lp = lm_fuse(lp, weight, trow[w]);
    const float t = lp0 + lp;
    const int ls = n0 + ((!f && w != end_id) ? 1 : 0);
    to[w] = t;
    sc[w] = t / pen[ls];
  }
}

void launch_las_beam_score(const float* logits, int Cp, int C, const float* logp, const int32_t* len, const int32_t* fin,
                           const float* pen, int end_id, int nrows, const float* table, const int32_t* ctx, float weight,
                           float* scores, float* totals, const int32_t* done, hipStream_t st) {
  hipLaunchKernelGGL(las_beam_score_kernel, dim3((nrows + 3) / 4), dim3(256), 0, st, logits, Cp, C, logp, len, fin, pen, end_id,
                     nrows, table, ctx, weight, scores, totals, done);
}

// The exact top-W of utterance b's N = W*C scores (block b, 1024 threads), in tf.nn.top_k's order: score descending, equal
// scores by flat index ascending.  Every candidate is the distinct 64-bit key (ord(score) << 32 | ~index); a radix select
// over 8-bit digits, most significant first, finds the bits P above digit position s such that exactly W keys have
// (key >> s) >= P (it stops at the first digit where the bin holding the W-th key holds exactly the keys still needed),
// the survivors are collected and bitonic-sorted in LDS.  Histogram counts are integer LDS atomics (one histogram per
// wave); the survivors' collection order does not matter since the sort of distinct keys fixes it.
constexpr int LAS_SEL_THREADS = 1024;
__global__ __launch_bounds__(LAS_SEL_THREADS) void las_beam_select_kernel(const float* __restrict__ scores, int W, int C,
                                                                          int32_t* __restrict__ sel_idx,
                                                                          float* __restrict__ sel_score,
                                                                          const int32_t* __restrict__ done) {
  __shared__ uint32_t hist[LAS_SEL_THREADS / 64][256];
  __shared__ uint32_t suf[256];
  __shared__ unsigned long long keys[LAS_SEL_THREADS];
  __shared__ unsigned long long s_prefix;
  __shared__ int s_need, s_stop, s_count;
  if (*done) return;
  const int b = blockIdx.x, tid = threadIdx.x, wv = tid >> 6;
  const int N = W * C;
  const float* sc = scores + (size_t)b * N;
  if (tid == 0) { s_prefix = 0ull; s_need = W; s_stop = 0; s_count = 0; }
  int s = 64;
  for (;;) {
    s -= 8;
    for (int i = tid; i < (LAS_SEL_THREADS / 64) * 256; i += LAS_SEL_THREADS) (&hist[0][0])[i] = 0u;
    __syncthreads();
    const unsigned long long P = s_prefix;
    const int need = s_need;
    for (int i = tid; i < N; i += LAS_SEL_THREADS) {
      const unsigned long long key = ((unsigned long long)ord_key(sc[i]) << 32) | (uint32_t)~(uint32_t)i;
      if (s == 56 || (key >> (s + 8)) == P) atomicAdd(&hist[wv][(uint32_t)(key >> s) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 256) {
      uint32_t n = 0;
      for (int q = 0; q < LAS_SEL_THREADS / 64; ++q) n += hist[q][tid];
      suf[tid] = n;
    }
    __syncthreads();
    // suffix sums: suf[j] = keys in bins >= j (Hillis-Steele, 8 rounds)
    for (int o = 1; o < 256; o <<= 1) {
      uint32_t add = 0;
      if (tid < 256 && tid + o < 256) add = suf[tid + o];
      __syncthreads();
      if (tid < 256) suf[tid] += add;
      __syncthreads();
    }
    if (tid < 256) {
      const uint32_t above = tid < 255 ? suf[tid + 1] : 0u;
      if (above < (uint32_t)need && suf[tid] >= (uint32_t)need) {   // bin tid holds the need-th key: exactly one thread
        const int rest = need - (int)above;
        s_prefix = (P << 8) | (unsigned long long)tid;
        s_need = rest;
        s_stop = (suf[tid] - above == (uint32_t)rest) || s == 0;
      }
    }
    __syncthreads();
    if (s_stop) break;
  }
  const unsigned long long P = s_prefix;
  keys[tid] = 0ull;   // below every real key (ord(-inf) << 32 > 0): the padding sorts last
  __syncthreads();
  for (int i = tid; i < N; i += LAS_SEL_THREADS) {
    const unsigned long long key = ((unsigned long long)ord_key(sc[i]) << 32) | (uint32_t)~(uint32_t)i;
    if ((key >> s) >= P) {
      const int pos = atomicAdd(&s_count, 1);
      if (pos < LAS_SEL_THREADS) keys[pos] = key;
    }
  }
  __syncthreads();
  for (int k = 2; k <= LAS_SEL_THREADS; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int p = tid ^ j;
      if (p > tid) {
        const unsigned long long a = keys[tid], c = keys[p];
        const bool desc = (tid & k) == 0;
        if (desc ? a < c : a > c) { keys[tid] = c; keys[p] = a; }
      }
      __syncthreads();
    }
  if (tid < W) {
    const unsigned long long key = keys[tid];
    sel_idx[(size_t)b * W + tid] = (int32_t)~(uint32_t)key;
    sel_score[(size_t)b * W + tid] = ord_val((uint32_t)(key >> 32));
  }
}

void launch_las_beam_select(const float* scores, int B, int W, int C, int32_t* sel_idx, float* sel_score, const int32_t* done,
                            hipStream_t st) {
  hipLaunchKernelGGL(las_beam_select_kernel, dim3(B), dim3(LAS_SEL_THREADS), 0, st, scores, W, C, sel_idx, sel_score, done);
}

// Beam row r = b*W + k takes candidate sel_idx[r] = parent*C + word: [a | h] and c gathered from the parent's row of the
// step's outputs (Sx, cx) into S, c; log_probs = total, finished = finished[parent] || word == end_id, lengths =
// lengths[parent] + !finished[parent]; ctx = finished[parent] ? ctx[parent] : (ctx[parent]*C + word) mod K (ctx_in: the
// step's input copy, as len_in / fin_in); the next input id; the trace row of the step (block r, 256 threads).
__global__ __launch_bounds__(256) void las_beam_update_kernel(
    const int32_t* __restrict__ sel_idx, const float* __restrict__ sel_score, const float* __restrict__ totals, int W, int C,
    int end_id, const float* __restrict__ Sx, const float* __restrict__ cx, const int32_t* __restrict__ len_in, const int32_t* __restrict__ fin_in, const int32_t* __restrict__ ctx_in, int K, float* __restrict__ S, float* __restrict__ c,
    int32_t* __restrict__ ids, float* __restrict__ logp_out, int32_t* __restrict__ len_out, int32_t* __restrict__ fin_out, int32_t* __restrict__ ctx_out,
    float* __restrict__ tr_score, int32_t* __restrict__ tr_word, int32_t* __restrict__ tr_parent,
    const int32_t* __restrict__ done) {
  if (*done) return;
  const int r = blockIdx.x, tid = threadIdx.x;
  const int b = r / W;
  int idx = sel_idx[r];
  if (idx < 0 || idx >= W * C) idx = 0;   // (the selection always writes a candidate; never index outside the rows)
  const int parent = idx / C, word = idx % C;
  const size_t pr = (size_t)b * W + parent;
  for (int k = tid; k < LAS_SW; k += blockDim.x) S[(size_t)r * LAS_SW + k] = Sx[pr * LAS_SW + k];
  for (int k = tid; k < LAS_HD; k += blockDim.x) c[(size_t)r * LAS_HD + k] = cx[pr * LAS_HD + k];
  if (tid == 0) {
    const int pf = fin_in[pr];
    logp_out[r] = totals[(size_t)b * W * C + idx];
    fin_out[r] = pf || word == end_id;
    len_out[r] = len_in[pr] + (pf ? 0 : 1);
    const int pc = ctx_in[pr];   // < K, and K * C <= 2^24: no overflow below
    ctx_out[r] = pf ? pc : (pc * C + word) % K;
    ids[r] = word;
    tr_score[r] = sel_score[r];
    tr_word[r] = word;
    tr_parent[r] = parent;
  }
}

void launch_las_beam_update(const int32_t* sel_idx, const float* sel_score, const float* totals, int W, int C, int end_id,
                            int nrows, const float* Sx, const float* cx, const int32_t* len_in,
                            const int32_t* fin_in, const int32_t* ctx_in, int K, float* S, float* c, int32_t* ids,
                            float* logp_out, int32_t* len_out, int32_t* fin_out, int32_t* ctx_out, float* tr_score,
                            int32_t* tr_word, int32_t* tr_parent, const int32_t* done, hipStream_t st) {
  hipLaunchKernelGGL(las_beam_update_kernel, dim3(nrows), dim3(256), 0, st, sel_idx, sel_score, totals, W, C, end_id, Sx, cx,
                     len_in, fin_in, ctx_in, K, S, c, ids, logp_out, len_out, fin_out, ctx_out, tr_score, tr_word, tr_parent,
                     done);
}

// after step t: flags[1] = t + 1 (steps run); flags[0] = 1 once every beam is finished or t + 1 == max_steps (one block)
__global__ __launch_bounds__(1024) void las_beam_finish_kernel(const int32_t* __restrict__ fin, int nrows, int t, int max_steps,
                                                               int32_t* __restrict__ flags) {
  if (flags[0]) return;
  int all = 1;
  for (int r = threadIdx.x; r < nrows; r += blockDim.x) all &= fin[r] != 0;
  all = __syncthreads_and(all);
  if (threadIdx.x == 0) {
    flags[1] = t + 1;
    if (all || t + 1 >= max_steps) flags[0] = 1;
  }
}

void launch_las_beam_finish(const int32_t* fin, int nrows, int t, int max_steps, int32_t* flags, hipStream_t st) {
  hipLaunchKernelGGL(las_beam_finish_kernel, dim3(1), dim3(1024), 0, st, fin, nrows, t, max_steps, flags);
}

// gather_tree (TF 1.15's kernel) of utterance b (block b): max_len = min(Tdec, max over beams of the final lengths); the
// output starts as end_id; beam k takes word[max_len-1][k], then walks the parents back to time 0 from beam k of the
// final order; every position after the first end_id (below max_len) becomes end_id.  word / parent / out [Tdec][B*W].
__global__ __launch_bounds__(1024) void las_beam_gather_tree_kernel(const int32_t* __restrict__ word,
                                                                    const int32_t* __restrict__ parent,
                                                                    const int32_t* __restrict__ len, int Tdec, int W, int nrows,
                                                                    int end_id, int32_t* __restrict__ out) {
  __shared__ int s_max;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) s_max = 0;
  __syncthreads();
  int m = 0;
  for (int k = tid; k < W; k += blockDim.x) m = max(m, len[(size_t)b * W + k]);
  atomicMax(&s_max, m);
  __syncthreads();
  const int ml = min(Tdec, s_max);
  for (int k = tid; k < W; k += blockDim.x) {
    const size_t col = (size_t)b * W + k;
    for (int t = 0; t < Tdec; ++t) out[(size_t)t * nrows + col] = end_id;
    if (ml <= 0) continue;
    out[(size_t)(ml - 1) * nrows + col] = word[(size_t)(ml - 1) * nrows + col];
    int p = parent[(size_t)(ml - 1) * nrows + col];
    for (int t = ml - 2; t >= 0; --t) {
      if (p < 0 || p >= W) { out[(size_t)t * nrows + col] = -1; break; }
      out[(size_t)t * nrows + col] = word[(size_t)t * nrows + (size_t)b * W + p];
      p = parent[(size_t)t * nrows + (size_t)b * W + p];
    }
    bool f = false;
    for (int t = 0; t < ml; ++t) {
      int32_t* o = out + (size_t)t * nrows + col;
      if (f) *o = end_id;
      else if (*o == end_id) f = true;
    }
  }
}

void launch_las_beam_gather_tree(const int32_t* word, const int32_t* parent, const int32_t* len, int Tdec, int B, int W,
                                 int end_id, int32_t* out, hipStream_t st) {
  hipLaunchKernelGGL(las_beam_gather_tree_kernel, dim3(B), dim3(1024), 0, st, word, parent, len, Tdec, W, B * W, end_id, out);
}

}  // namespace nasr
