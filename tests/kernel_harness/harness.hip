// harness.hip — test-only C entry points over kernels.h for the GEMM layer (gemm.hip, gemm_tph.hip, the reductions of
// optim.hip).  Linked into neuralasr_amd/libnasr_kt.so with the SAME gemm.o / gemm_tph.o / optim.o objects as libnasr.so
// (neuralasr_amd/build.py), so the tests run the shipped code objects.  Every call takes host pointers, allocates,
// uploads, launches on one stream, synchronises, copies back and frees; it returns the HIP error code, 0, or -1 for
// arguments whose buffers would not cover what the kernel touches.  Output, plane and slab buffers are pre-filled with
// a caller-given byte, so a test can tell which bytes a kernel left alone.  tests/kernel_harness.py is the ctypes side.
// The recurrence launchers (lstm.hip, lstm_persist.hip, lstm_wide.hip) have their entry points in rec_harness.hip, built
// into the same library; arena.h holds what the two files share.
#include "../../neuralasr_amd/csrc/kernels.h"
#include "arena.h"

#include <vector>

using namespace nasr;

extern "C" {

// ---- host-side choices of the launchers
int kt_gemm_pick_split(int M, int N, int K) { return gemm_pick_split(M, N, K); }
int kt_gemm_tp_tile_rows(int M) { return gemm_tp_tile_rows(M); }
int kt_gemm_tph_pick_split(int M, int N, int K, int nbatch) { return gemm_tph_pick_split(M, N, K, nbatch); }
int kt_tp_split2_parts(int rows) { return tp_split2_parts(rows); }
unsigned long long kt_tph_bytes(int rows, int K) { return tph_bytes(rows, K); }

// ---- gemm.hip
struct KtGemm {
  int M, N, K, lda, ldb, ldc, a_col, b_col, a_shift, a_rows, split_k;
};
// A: a_floats, B: b_floats, C: c_floats host floats (C comes back whole); a_map / c_map / bias may be NULL
int kt_gemm_f32(const KtGemm* d, const float* A, long long a_floats, const float* B, long long b_floats, float* C,
                long long c_floats, const int* a_map, int a_map_n, const int* c_map, const float* bias, int fill) {
  const long long a_w = d->a_col ? d->M : d->K, b_rows = d->b_col ? d->N : d->K, b_w = d->b_col ? d->K : d->N;
  if (d->a_rows > 0 && a_floats < (long long)(d->a_rows - 1) * d->lda + a_w) return -1;
  if (b_floats < (b_rows - 1) * d->ldb + b_w) return -1;
  if (a_map && a_map_n < (d->a_col ? d->K : d->M)) return -1;
  long long top = d->M - 1;
  if (c_map) {
    top = -1;
    for (int i = 0; i < d->M; ++i) top = c_map[i] > top ? c_map[i] : top;
  }
  if (top >= 0 && c_floats < top * d->ldc + d->N) return -1;
  Arena a;
  GemmDesc g{};
  g.A = a.up(A, a_floats); g.B = a.up(B, b_floats);
  float* dC = a.filled<float>(c_floats, fill);
  g.C = dC;
  g.M = d->M; g.N = d->N; g.K = d->K; g.lda = d->lda; g.ldb = d->ldb; g.ldc = d->ldc;
  g.a_col = d->a_col != 0; g.b_col = d->b_col != 0;
  g.a_map = a.up(a_map, a_map_n); g.a_shift = d->a_shift; g.a_rows = d->a_rows;
  g.c_map = a.up(c_map, d->M); g.bias = a.up(bias, d->N);
  g.split_k = d->split_k;
  g.slabs = d->split_k > 1 ? a.filled<float>((size_t)d->split_k * d->M * d->N, 0xFF) : nullptr;   // NaN until written
  if (a.err == hipSuccess) launch_gemm(g, a.st);
  a.down(C, dC, c_floats);
  return a.finish();
}

// ---- gemm_tph.hip: scales
int kt_tph_scales(const float* src, long long src_floats, int rows, int K, int ld, float* row_scale, float* row_inv,
                  float* col_scale, float* col_inv, int fill) {
  if (src_floats < (long long)(rows - 1) * ld + K) return -1;
  Arena a;
  const float* s = a.up(src, src_floats);
  float* rs = row_scale ? a.filled<float>(rows, fill) : nullptr;
  float* ri = row_scale ? a.filled<float>(rows, fill) : nullptr;
  float* cs = col_scale ? a.filled<float>(K, fill) : nullptr;
  float* ci = col_scale ? a.filled<float>(K, fill) : nullptr;
  float* ws = a.filled<float>(tph_scale_ws_floats(rows, K), 0xFF);
  if (a.err == hipSuccess) launch_tph_scales(s, rows, K, ld, rs, ri, cs, ci, ws, a.st);
  a.down(row_scale, rs, rows); a.down(row_inv, ri, rows); a.down(col_scale, cs, K); a.down(col_inv, ci, K);
  return a.finish();
}

struct KtScaleJob {
  const float* src;
  long long src_floats;
  int rows, K, ld, pad;
  float *row_scale, *row_inv, *col_scale, *col_inv;     // row pair may be NULL; the column pair is always written
};
int kt_tph_scales_batch(const KtScaleJob* jobs, int n, int fill) {
  Arena a;
  std::vector<TphScaleJob> dj(n);
  for (int i = 0; i < n; ++i) {
    const KtScaleJob& q = jobs[i];
    if (q.src_floats < (long long)(q.rows - 1) * q.ld + q.K || !q.col_scale || !q.col_inv) return -1;
    dj[i] = TphScaleJob{a.up(q.src, q.src_floats), q.rows, q.K, q.ld,
                        q.row_scale ? a.filled<float>(q.rows, fill) : nullptr, q.row_scale ? a.filled<float>(q.rows, fill) : nullptr,
                        a.filled<float>(q.K, fill), a.filled<float>(q.K, fill)};
  }
  float* ws = a.filled<float>(tph_scale_batch_ws_floats(dj.data(), n), 0xFF);
  if (a.err == hipSuccess) launch_tph_scales_batch(dj.data(), n, ws, a.st);
  for (int i = 0; i < n; ++i) {
    a.down(jobs[i].row_scale, dj[i].row_scale, jobs[i].rows); a.down(jobs[i].row_inv, dj[i].row_inv, jobs[i].rows);
    a.down(jobs[i].col_scale, dj[i].col_scale, jobs[i].K); a.down(jobs[i].col_inv, dj[i].col_inv, jobs[i].K);
  }
  return a.finish();
}

// rowpart [nrp][rows] -> row_scale / row_inv, colpart [ncp][K] -> col_scale / col_inv; either side may be NULL
int kt_tph_scales_from_parts(const float* rowpart, int nrp, int rows, float* row_scale, float* row_inv, const float* colpart,
                             int ncp, int K, float* col_scale, float* col_inv, int fill) {
  Arena a;
  const float* rp = a.up(rowpart, (size_t)nrp * rows);
  const float* cp = a.up(colpart, (size_t)ncp * K);
  float* rs = rowpart ? a.filled<float>(rows, fill) : nullptr;
  float* ri = rowpart ? a.filled<float>(rows, fill) : nullptr;
  float* cs = colpart ? a.filled<float>(K, fill) : nullptr;
  float* ci = colpart ? a.filled<float>(K, fill) : nullptr;
  if (a.err == hipSuccess) launch_tph_scales_from_parts(rp, nrp, rows, rs, ri, cp, ncp, K, cs, ci, a.st);
  a.down(row_scale, rs, rows); a.down(row_inv, ri, rows); a.down(col_scale, cs, K); a.down(col_inv, ci, K);
  return a.finish();
}

// ---- gemm_tph.hip: fp32 -> planes.  src: src_rows physical rows of ld floats.  tpN (tph_bytes(rows, K)), tpT
// (tph_bytes(K, rows)) and colpart (tp_split2_parts(rows) x K) are optional outputs; row_scale [rows] / col_scale [K]
// NULL: the constants rs / cs.  rowmap / rowmap2 [rows] or NULL.
int kt_tph_split2(const float* src, int src_rows, int rows, int K, int ld, const float* row_scale, float rs,
                  const float* col_scale, float cs, unsigned char* tpN, unsigned char* tpT, float* colpart, const int* rowmap,
                  const int* rowmap2, int col2, int fill) {
  if (ld < K || (!rowmap && src_rows < rows)) return -1;
  for (int i = 0; i < rows; ++i)
    if ((rowmap && rowmap[i] >= src_rows) || (rowmap2 && rowmap2[i] >= src_rows)) return -1;
  Arena a;
  const float* s = a.up(src, (size_t)src_rows * ld);
  const size_t nN = tph_bytes(rows, K), nT = tph_bytes(K, rows), nC = (size_t)tp_split2_parts(rows) * K;
  unsigned char* dN = tpN ? a.filled<unsigned char>(nN, fill) : nullptr;
  unsigned char* dT = tpT ? a.filled<unsigned char>(nT, fill) : nullptr;
  float* dC = colpart ? a.filled<float>(nC, fill) : nullptr;
  const float* drs = a.up(row_scale, rows);
  const float* dcs = a.up(col_scale, K);
  const int* m1 = a.up(rowmap, rows);
  const int* m2 = a.up(rowmap2, rows);
  if (a.err == hipSuccess) launch_tph_split2(s, dN, dT, rows, K, ld, drs, rs, dcs, cs, dC, a.st, m1, m2, col2);
  a.down(tpN, dN, nN); a.down(tpT, dT, nT); a.down(colpart, dC, nC);
  return a.finish();
}

// ---- gemm_tph.hip: the GEMM.  Operands either as planes (A_tp / B_tp: bytes uploaded as given, with a_inv / b_inv) or as
// fp32 matrices A32 [a_rows][KA], B32 [b_rows][KB] that the harness turns into planes with launch_tph_scales (row scales)
// and launch_tph_split2 - the path the library takes.  Batch 1 of nbatch == 2 lives in the same buffers, at the strides.
struct KtTph {
  int M, N, K, KA, KB, ldc, a_kshift, a_kshift1, split_k, tile_rows, nbatch, side;
  long long a_bstride, b_bstride, c_bstride, ainv_bstride, binv_bstride;     // a_/b_bstride in bytes
  int a_rows, b_rows;       // fp32 form: rows of A32 / B32 (both batches); plane form: rows the inverse scales cover
};
int kt_gemm_tph(const KtTph* d, const float* A32, const float* B32, const unsigned char* A_tp, long long a_bytes,
                const unsigned char* B_tp, long long b_bytes, const float* a_inv, const float* b_inv, float* C,
                long long c_floats, const float* bias, const int* c_map, int fill) {
  const int nb = d->nbatch > 1 ? 2 : 1;
  const int nkbA = (d->KA + 15) / 16, nkbB = (d->KB + 15) / 16;
  Arena a;
  const unsigned char *dA, *dB;
  const float *dai, *dbi;
  if (A32) {
    if (!B32) return -1;
    a_bytes = (long long)tph_bytes(d->a_rows, d->KA); b_bytes = (long long)tph_bytes(d->b_rows, d->KB);
    float* sc[4];
    unsigned char* tp[2];
    for (int o = 0; o < 2; ++o) {
      const int rows = o ? d->b_rows : d->a_rows, K = o ? d->KB : d->KA;
      const float* s = a.up(o ? B32 : A32, (size_t)rows * K);
      sc[2 * o] = a.filled<float>(rows, 0xFF); sc[2 * o + 1] = a.filled<float>(rows, 0xFF);
      float* ws = a.filled<float>(tph_scale_ws_floats(rows, K), 0xFF);
      tp[o] = a.filled<unsigned char>(o ? b_bytes : a_bytes, fill);
      if (a.err != hipSuccess) return (int)a.err;
      launch_tph_scales(s, rows, K, K, sc[2 * o], sc[2 * o + 1], nullptr, nullptr, ws, a.st);
      launch_tph_split2(s, tp[o], nullptr, rows, K, K, sc[2 * o], 1.f, nullptr, 1.f, nullptr, a.st);
    }
    dA = tp[0]; dB = tp[1]; dai = sc[1]; dbi = sc[3];
  } else {
    if (!A_tp || !B_tp || !a_inv || !b_inv) return -1;
    dA = a.up(A_tp, a_bytes); dB = a.up(B_tp, b_bytes);
    dai = a.up(a_inv, d->a_rows); dbi = a.up(b_inv, d->b_rows);
  }
  // what the kernel touches: whole row blocks of the operands, M / N inverse scales per batch, the result rows
  if (a_bytes < (long long)(nb - 1) * d->a_bstride + (long long)rup(d->M, 32) / 32 * nkbA * 2048) return -1;
  if (b_bytes < (long long)(nb - 1) * d->b_bstride + (long long)rup(d->N, 32) / 32 * nkbB * 2048) return -1;
  if (d->a_rows < (nb - 1) * d->ainv_bstride + d->M || d->b_rows < (nb - 1) * d->binv_bstride + d->N) return -1;
  long long top = d->M - 1;
  if (c_map && !d->side) {
    top = -1;
    for (int i = 0; i < d->M; ++i) top = c_map[i] > top ? c_map[i] : top;
  }
  if (d->split_k > 1 && !c_map && d->ldc != d->N) return -1;
  if (top >= 0 && c_floats < (nb - 1) * d->c_bstride + top * d->ldc + d->N) return -1;
  if (c_map && nb > 1) return -1;
  if (!a.chk(gemm_tph_prepare())) return (int)a.err;
  GemmTPHDesc g{};
  g.A = dA; g.B = dB;
  float* dC = a.filled<float>(c_floats, fill);
  g.C = dC;
  g.M = d->M; g.N = d->N; g.K = d->K; g.nkbA = nkbA; g.nkbB = nkbB; g.ldc = d->ldc;
  g.a_kshift = d->a_kshift; g.a_kshift1 = d->a_kshift1;
  g.bias = a.up(bias, d->N); g.a_inv = dai; g.b_inv = dbi;
  g.split_k = d->split_k;
  g.slabs = d->split_k > 1 ? a.filled<float>((size_t)nb * d->split_k * d->M * d->N, 0xFF) : nullptr;
  g.tile_rows = d->tile_rows; g.nbatch = d->nbatch; g.side = d->side != 0;
  g.a_bstride = (size_t)d->a_bstride; g.b_bstride = (size_t)d->b_bstride; g.c_bstride = d->c_bstride;
  g.ainv_bstride = d->ainv_bstride; g.binv_bstride = d->binv_bstride;
  g.c_map = a.up(c_map, d->M);
  if (a.err == hipSuccess) launch_gemm_tph(g, a.st);
  a.down(C, dC, c_floats);
  return a.finish();
}

// ---- optim.hip: the reductions behind the GEMMs
int kt_colsum(const float* M, int R, int N, int ld, float* out, int out_floats, int fill) {
  if (ld < N || out_floats < N) return -1;
  Arena a;
  const float* s = a.up(M, (size_t)R * ld);
  float* o = a.filled<float>(out_floats, fill);
  float* ws = a.filled<float>((size_t)32 * N, 0xFF);
  if (a.err == hipSuccess) launch_colsum(s, R, N, ld, o, ws, a.st);
  a.down(out, o, out_floats);
  return a.finish();
}
int kt_colsum_parts(const float* part, int nparts, int N, float* out, int out_floats, int fill) {
  if (out_floats < N) return -1;
  Arena a;
  const float* s = a.up(part, (size_t)nparts * N);
  float* o = a.filled<float>(out_floats, fill);
  if (a.err == hipSuccess) launch_colsum_parts(s, nparts, N, o, a.st);
  a.down(out, o, out_floats);
  return a.finish();
}
int kt_reduce_slabs(const float* slabs, int S, long long n, float* out, long long out_floats, int fill) {
  if (out_floats < n) return -1;
  Arena a;
  const float* s = a.up(slabs, (size_t)S * n);
  float* o = a.filled<float>(out_floats, fill);
  if (a.err == hipSuccess) launch_reduce_slabs(s, S, n, o, a.st);
  a.down(out, o, out_floats);
  return a.finish();
}
int kt_reduce_slabs_rows(const float* slabs, int S, int M, int N, int ldc, const int* map, float* out, long long out_floats,
                         int fill) {
  if (!map || ldc < N) return -1;
  for (int i = 0; i < M; ++i)
    if (map[i] >= 0 && out_floats < (long long)map[i] * ldc + N) return -1;
  Arena a;
  const float* s = a.up(slabs, (size_t)S * M * N);
  const int* m = a.up(map, M);
  float* o = a.filled<float>(out_floats, fill);
  if (a.err == hipSuccess) launch_reduce_slabs_rows(s, S, M, N, ldc, m, o, a.st);
  a.down(out, o, out_floats);
  return a.finish();
}

}  // extern "C"
