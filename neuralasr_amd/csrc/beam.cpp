// beam.cpp — tf.nn.ctc_beam_search_decoder (networks/tfnetwork.py:61-64: defaults beam_width = 100,
// top_paths = 1, merge_repeated = True) as host code: prefix beam search over per-frame log-softmax, a beam
// entry carrying (p_blank, p_label, p_total) of its prefix, at most `beam_width` live entries per frame
// (SURVEY.md Appendix A.6).  merge_repeated additionally merges adjacent equal labels of the OUTPUT sequence,
// even when a blank separated them (TF's documented quirk).  One thread per utterance.
// Parity status: restated from TF 1.x's documented algorithm; unpinned (no TF here), cross-checked against an
// independent Python restatement (oracle/nasr_oracle.py: ctc_beam_search) in tests/test_beam.py.
//
// nasr_ctc_beam_search_lm fuses a dense n-gram table over the label ids: every entry carries the context
// index of its prefix, and wherever mass flows from an entry to its extension by label c that contribution gets
// weight * logp[ctx(parent)][c] + bonus; the top path is chosen by total + weight * eos[ctx].  The plain call is the same
// code with no table.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <deque>
#include <limits>
#include <memory>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/nasr.h"

namespace {

constexpr float kLogZero = -std::numeric_limits<float>::infinity();

inline float lse(float a, float b) {
  if (a == kLogZero) return b;
  if (b == kLogZero) return a;
  return a > b ? a + std::log1p(std::exp(b - a)) : b + std::log1p(std::exp(a - b));
}

struct Prob {
  float total = kLogZero, blank = kLogZero, label = kLogZero;
  void reset() { total = blank = label = kLogZero; }
};

// One prefix of the beam tree.  Children sit in a flat array indexed by label, allocated from the decoder's arena on the
// first extension (a hash map per entry and a heap allocation per child made the decoder 5-10x slower than this).
struct Entry {
  Entry* parent = nullptr;
  int label = -1;
  int ctx = 0;   // the n-gram context index of this prefix (Lm)
  Prob oldp, newp;
  Entry** kids = nullptr;
  bool active() const { return newp.total != kLogZero; }
};

// The n-gram table of a fused search: logp [K][C], eos [K], K = C^(order-1); a context is the last order-1 ids with the
// most recent as the lowest digit.  No table (logp == nullptr): every term below is skipped, not added as zero.
struct Lm {
  const float* logp = nullptr;
  const float* eos = nullptr;
  int C = 0, K = 1, root = 0;
  float weight = 0.f, bonus = 0.f;
  // what an extension of a prefix with context ctx by label c adds to the mass it carries over
  float step(int ctx, int c) const { return weight * logp[(size_t)ctx * C + c] + bonus; }
  int next(int ctx, int c) const { return (int)(((int64_t)ctx * C + c) % K); }
  float final_score(const Entry* e) const { return logp ? e->newp.total + weight * eos[e->ctx] : e->newp.total; }
};

struct Arena {
  int C;
  const Lm& lm;
  std::deque<Entry> entries;
  std::deque<std::vector<Entry*>> kid_arrays;
  Arena(int c, const Lm& l) : C(c), lm(l) {}
  Entry* child(Entry* p, int lab) {
    if (!p->kids) {
      kid_arrays.emplace_back((size_t)C, nullptr);
      p->kids = kid_arrays.back().data();
    }
    Entry*& slot = p->kids[lab];
    if (!slot) {
      entries.emplace_back();
      slot = &entries.back();
      slot->parent = p;
      slot->label = lab;
      if (lm.logp) slot->ctx = lm.next(p->ctx, lab);
    }
    return slot;
  }
};

// bounded "top N by newp.total" container: a min-heap on the total, so the bottom is the front and a push that evicts it
// costs O(log N) (the entries' totals do not change while they sit in it)
struct Leaves {
  size_t cap;
  std::vector<Entry*> v;
  explicit Leaves(size_t c) : cap(c) {}
  static bool better(const Entry* a, const Entry* b) { return a->newp.total > b->newp.total; }
  Entry* bottom() const { return v.front(); }
  void push(Entry* e) {
    if (v.size() < cap) {
      v.push_back(e);
      std::push_heap(v.begin(), v.end(), better);
      return;
    }
    if (e->newp.total > v.front()->newp.total) {
      std::pop_heap(v.begin(), v.end(), better);
      v.back() = e;
      std::push_heap(v.begin(), v.end(), better);
    }
  }
};

// The search as a state that lives between calls: the beam tree (arena, root, leaves) after the frames fed so far.
// feed() is TF's per-frame procedure, one frame after the other with no look-ahead; best() is a non-destructive maximum
// over the leaves, so a search can be asked at any time and then go on.  The whole-utterance calls are open + one feed +
// best (decode_one); nasr_ctc_beam_open / feed / best / close hand the same object out (one handle per thread).
struct Search {
  int C, blank;
  bool merge_repeated;
  Lm lm;
  Arena arena;
  Entry root;
  Leaves leaves;
  std::vector<float> lp;
  Search(int c, int beam_width, bool merge, const Lm& l)
      : C(c), blank(c - 1), merge_repeated(merge), lm(l), arena(c, lm), leaves((size_t)beam_width), lp((size_t)c) {
    root.ctx = lm.root;
    root.newp.total = 0.f;
    root.newp.blank = 0.f;
    leaves.v.push_back(&root);
  }
  Search(const Search&) = delete;
  Search& operator=(const Search&) = delete;

  void feed(const float* logits, size_t frame_stride, int T) {
    for (int t = 0; t < T; ++t) {
      const float* x = logits + (size_t)t * frame_stride;
      float m = x[0];
      for (int c = 1; c < C; ++c) m = std::max(m, x[c]);
      double s = 0.0;
      for (int c = 0; c < C; ++c) s += std::exp((double)x[c] - m);
      const float norm = m + (float)std::log(s);
      for (int c = 0; c < C; ++c) lp[c] = x[c] - norm;

      std::vector<Entry*> branches = leaves.v;
      std::sort(branches.begin(), branches.end(), Leaves::better);
      leaves.v.clear();
      for (Entry* b : branches) b->oldp = b->newp;
      for (Entry* b : branches) {   // extensions that keep the prefix
        if (b->parent) {
          if (b->parent->active()) {
            float prev = (b->label == b->parent->label) ? b->parent->oldp.blank : b->parent->oldp.total;
            if (lm.logp) prev += lm.step(b->parent->ctx, b->label);
            b->newp.label = lse(b->newp.label, prev);
          }
          b->newp.label += lp[b->label];
        }
        b->newp.blank = b->oldp.total + lp[blank];
        b->newp.total = lse(b->newp.blank, b->newp.label);
        leaves.push(b);
      }
      for (Entry* b : branches) {   // grow new leaves
        auto candidate = [&](const Prob& p) {
          return p.total > kLogZero && (leaves.v.size() < leaves.cap || p.total > leaves.bottom()->newp.total);
        };
        if (!candidate(b->oldp)) continue;
        for (int lab = 0; lab < C; ++lab) {
          if (lab == blank) continue;
          // the extension's score needs nothing of the child: test it against the beam's bottom BEFORE the child is looked up
          // or created (an inactive child that fails the test is left as it is: nothing reads it until it becomes a leaf)
          float prev = (lab == b->label) ? b->oldp.blank : b->oldp.total;
          if (lm.logp) prev += lm.step(b->ctx, lab);
          Prob np;
          np.blank = kLogZero;
          np.label = lp[lab] + prev;
          np.total = np.label;
          if (!candidate(np)) {
            // (TF's decoder clears BOTH probabilities of a child that fails here.  That matters for one kind of child: one that
            //  was a leaf of this frame, was evicted above and is still to come in this loop - cleared, it grows no children)
            Entry* e = b->kids ? b->kids[lab] : nullptr;
            if (e && !e->active()) e->oldp.reset();
            continue;
          }
          Entry* c = arena.child(b, lab);
          if (c->active()) continue;
          c->newp = np;
          if (leaves.v.size() == leaves.cap) leaves.bottom()->newp.reset();
          leaves.push(c);
        }
      }
    }
  }

  // the top path of the frames fed so far (the empty one before the first); reads the tree, changes nothing
  std::vector<int> best(float* logp_out) const {
    const Entry* top = *std::max_element(leaves.v.begin(), leaves.v.end(),
                                         [&](const Entry* a, const Entry* b) { return lm.final_score(a) < lm.final_score(b); });
    std::vector<int> seq;
    int prev_label = -1;
    for (const Entry* c = top; c->parent; c = c->parent) {
      if (!merge_repeated || c->label != prev_label) seq.push_back(c->label);
      prev_label = c->label;
    }
    std::reverse(seq.begin(), seq.end());
    if (logp_out) *logp_out = lm.final_score(top);
    return seq;
  }
};

void decode_one(const float* logits, size_t frame_stride, int T, int C, int beam_width, bool merge_repeated, const Lm& lm,
                int32_t* ids_out, int32_t* len_out, float* logp_out) {
  Search search(C, beam_width, merge_repeated, lm);
  search.feed(logits, frame_stride, T);
  const std::vector<int> seq = search.best(logp_out);
  *len_out = (int32_t)seq.size();
  for (size_t i = 0; i < seq.size(); ++i) ids_out[i] = seq[i];
}

int beam_search(const float* logits, const int32_t* seq_len, int B, int Tp, int C, int beam_width, int merge_repeated,
                const Lm& lm, int32_t* ids_out, int32_t* lens_out, float* logp_out) {
  if (!logits || !seq_len || !ids_out || !lens_out || B < 1 || Tp < 1 || C < 2 || beam_width < 1) return NASR_ERR_ARG;
  for (int b = 0; b < B; ++b)
    if (seq_len[b] < 0 || seq_len[b] > Tp) return NASR_ERR_ARG;
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  const int nthr = (int)std::min<unsigned>(hw, (unsigned)B);
  std::vector<std::thread> pool;
  for (int w = 0; w < nthr; ++w)
    pool.emplace_back([=, &lm]() {
      for (int b = w; b < B; b += nthr)
        decode_one(logits + (size_t)b * C, (size_t)B * C, seq_len[b], C, beam_width, merge_repeated != 0, lm,
                   ids_out + (size_t)b * Tp, lens_out + b, logp_out ? logp_out + b : nullptr);
    });
  for (auto& t : pool) t.join();
  return NASR_OK;
}

// the n-gram arguments of the ABI as an Lm (lm_logp == NULL: no table, the rest is not read); false: a bad argument
bool make_lm(int C, const float* lm_logp, const float* lm_eos, int order, int bos_id, float weight, float bonus, Lm* out) {
  Lm lm;
  if (lm_logp) {
    if (!lm_eos || C < 2 || order < 1 || order > 4 || bos_id < 0 || bos_id >= C) return false;
    int64_t K = 1;   // C^(order-1); the table's K * C entries may not exceed 2^24
    for (int i = 1; i < order && K * C <= ((int64_t)1 << 24); ++i) K *= C;
    if (K * C > ((int64_t)1 << 24)) return false;
    lm.logp = lm_logp; lm.eos = lm_eos; lm.C = C; lm.K = (int)K; lm.weight = weight; lm.bonus = bonus;
    for (int i = 1; i < order; ++i) lm.root = lm.root * C + bos_id;
  }
  *out = lm;
  return true;
}

}  // namespace

struct nasr_beam {
  Search search;
  nasr_beam(int C, int beam_width, bool merge, const Lm& lm) : search(C, beam_width, merge, lm) {}
};

extern "C" int nasr_ctc_beam_search(const float* logits, const int32_t* seq_len, int B, int Tp, int C, int beam_width,
                                    int merge_repeated, int32_t* ids_out, int32_t* lens_out, float* logp_out) {
  return beam_search(logits, seq_len, B, Tp, C, beam_width, merge_repeated, Lm(), ids_out, lens_out, logp_out);
}

extern "C" int nasr_ctc_beam_search_lm(const float* logits, const int32_t* seq_len, int B, int Tp, int C, int beam_width,
                                       int merge_repeated, const float* lm_logp, const float* lm_eos, int order, int bos_id,
                                       float weight, float bonus, int32_t* ids_out, int32_t* lens_out, float* logp_out) {
  Lm lm;
  if (!make_lm(C, lm_logp, lm_eos, order, bos_id, weight, bonus, &lm)) return NASR_ERR_ARG;
  return beam_search(logits, seq_len, B, Tp, C, beam_width, merge_repeated, lm, ids_out, lens_out, logp_out);
}

extern "C" int nasr_ctc_beam_open(int C, int beam_width, int merge_repeated, const float* lm_logp, const float* lm_eos, int order,
                                  int bos_id, float weight, float bonus, nasr_beam_handle* out) {
  if (!out) return NASR_ERR_ARG;
  *out = nullptr;
  Lm lm;
  if (C < 2 || beam_width < 1 || !make_lm(C, lm_logp, lm_eos, order, bos_id, weight, bonus, &lm)) return NASR_ERR_ARG;
  *out = new nasr_beam(C, beam_width, merge_repeated != 0, lm);
  return NASR_OK;
}

extern "C" int nasr_ctc_beam_feed(nasr_beam_handle s, const float* logits, int64_t frame_stride, int n_frames) {
  if (!s || n_frames < 0 || (n_frames > 0 && (!logits || frame_stride < s->search.C))) return NASR_ERR_ARG;
  s->search.feed(logits, (size_t)frame_stride, n_frames);
  return NASR_OK;
}

extern "C" int nasr_ctc_beam_best(nasr_beam_handle s, int32_t* ids_out, int cap, int32_t* len_out, float* logp_out) {
  if (!s || !len_out || cap < 0 || (cap > 0 && !ids_out)) return NASR_ERR_ARG;
  float logp = 0.f;
  const std::vector<int> seq = s->search.best(&logp);
  *len_out = (int32_t)seq.size();
  if (logp_out) *logp_out = logp;
  if (seq.size() > (size_t)cap) return NASR_ERR_ARG;
  for (size_t i = 0; i < seq.size(); ++i) ids_out[i] = seq[i];
  return NASR_OK;
}

extern "C" int nasr_ctc_beam_close(nasr_beam_handle s) {
  delete s;
  return NASR_OK;
}
