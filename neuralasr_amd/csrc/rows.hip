// rows.hip — the row movers around the recurrence: kernels that only copy rows from one order into another, zeros where the
// source has none.  Feature packing and context expansion, the window assembly of a look-ahead stream session (DESIGN.md
// §18), the gather / emit / scatter between frames and the windows of latency-controlled training (§19).  No arithmetic.
#include "kernels.h"

namespace nasr {

// ------------------------------------------------------------------ feature transpose + pad
// feats [B][T][F] batch-major (dataset.py:75-82) -> X0 [(t*Bp+b)][Fp], zero padded.  With a frame skip
// network row t is input frame t*skip, and rows from the utterance's network length on - t*skip >= seq_in[b] - are zero;
// seq_in NULL (skip 1): the caller's rows as they are, padding included.
__global__ __launch_bounds__(256) void pack_feats_kernel(const float* __restrict__ f, float* __restrict__ x, int B,
                                                         int Bp, int T, int F, int Fp, int skip,
                                                         const int* __restrict__ seq_in) {
  const int r = blockIdx.x;  // t*Bp + b
  const int t = r / Bp, b = r % Bp;
  float* dst = x + (size_t)r * Fp;
  if (b >= B || (seq_in && t * skip >= seq_in[b])) {
    for (int i = threadIdx.x; i < Fp; i += blockDim.x) dst[i] = 0.f;
    return;
  }
  const float* src = f + ((size_t)b * T + (size_t)t * skip) * F;
  for (int i = threadIdx.x; i < Fp; i += blockDim.x) dst[i] = i < F ? src[i] : 0.f;
}

void launch_pack_feats(const float* feats_bm, float* X0, int B, int Bp, int T, int F, int Fp, hipStream_t st, int skip,
                       const int* seq_in) {
  hipLaunchKernelGGL(pack_feats_kernel, dim3(skip_frames(T, skip) * Bp), dim3(256), 0, st, feats_bm, X0, B, Bp, T, F, Fp, skip,
                     seq_in);
}

// include_context on the device (utils.py:8-21): the caller ships only the centre frame [B][T][numcep]; every
// time-major row gets its (2*ctx+1)-frame window, out-of-range frames of an utterance filled with that
// utterance's pad value (0 before the utterance-level normalisation of utils.py:29, (0-mean)/std after it),
// frames past seq_len zero (dataset.py:75-77).  21x fewer bytes over PCIe for numcontext = 10.
// With a frame skip network row t is input frame t*skip: its window is that input frame's, decided on input frame
// indices against the input length seq_len[b] (t*skip >= seq_len[b] is a row from the network length on: zero).
__global__ __launch_bounds__(256) void expand_context_kernel(const float* __restrict__ centre,
                                                             const float* __restrict__ pad, const int* __restrict__ seq_len,
                                                             float* __restrict__ x, int B, int Bp, int T, int ctx,
                                                             int ncep, int Fp, int skip) {
  const int r = blockIdx.x;  // t*Bp + b
  const int t = (r / Bp) * skip, b = r % Bp;   // t: the input frame
  float* dst = x + (size_t)r * Fp;
  const int len = b < B ? seq_len[b] : 0;
  const int F = (2 * ctx + 1) * ncep;
  for (int i = threadIdx.x; i < Fp; i += blockDim.x) {
    float v = 0.f;
    if (i < F && t < len) {
      const int wdw = i / ncep, c = i - wdw * ncep;
      const int ts = t + wdw - ctx;
      v = (ts >= 0 && ts < len) ? centre[((size_t)b * T + ts) * ncep + c] : pad[b];
    }
    dst[i] = v;
  }
}

void launch_expand_context(const float* centre, const float* pad, const int* seq_len, float* X0, int B, int Bp, int T,
                           int ctx, int ncep, int Fp, hipStream_t st, int skip) {
  hipLaunchKernelGGL(expand_context_kernel, dim3(skip_frames(T, skip) * Bp), dim3(256), 0, st, centre, pad, seq_len, X0, B, Bp,
                     T, ctx, ncep, Fp, skip);
}

// expand_context_kernel with SpecAugment masks (the reference has no augmentation but rand_shift): the
// masks are applied to the utterance's normalised centre frames - 0 is their mean - and include_context runs on the
// result, so a masked frame is masked in every window it appears in and the pads stay what they were.  masks [B][nm]:
// {t0, tw, f0, fw}, validated on the host to lie inside the utterance and the static block.  The row's workgroup
// decides one flag per window and one per column (the mask list is walked nw + ncep times, not once per element) and
// keeps them in LDS: flag [nw] windows | [ncep] columns.  The frame skip as in expand_context_kernel: the masks are in input
// frames, like every index the row decides on.
__global__ __launch_bounds__(256) void expand_context_masked_kernel(const float* __restrict__ centre,
                                                                    const float* __restrict__ pad,
                                                                    const int* __restrict__ seq_len,
                                                                    const int4* __restrict__ masks, int nm, int sw,
                                                                    float* __restrict__ x, int B, int Bp, int T, int ctx,
                                                                    int ncep, int Fp, int skip) {
  extern __shared__ __attribute__((aligned(16))) unsigned char flag[];
  const int r = blockIdx.x;  // t*Bp + b
  const int t = (r / Bp) * skip, b = r % Bp;   // t: the input frame
  float* dst = x + (size_t)r * Fp;
  const int len = b < B ? seq_len[b] : 0;
  if (t >= len) {            // (the whole workgroup: no barrier is skipped by a part of it)
    for (int i = threadIdx.x; i < Fp; i += blockDim.x) dst[i] = 0.f;
    return;
  }
  const int nw = 2 * ctx + 1, F = nw * ncep;
  const int4* mk = masks + (size_t)b * nm;
  for (int j = threadIdx.x; j < nw + ncep; j += blockDim.x) {
    bool hit = false;
    if (j < nw) {
      const int ts = t + j - ctx;     // outside [0, len): a pad, and no mask reaches there
      for (int k = 0; k < nm; ++k) hit |= ts >= mk[k].x && ts < mk[k].x + mk[k].y;
    } else {
      const int c = (j - nw) % sw;
      for (int k = 0; k < nm; ++k) hit |= c >= mk[k].z && c < mk[k].z + mk[k].w;
    }
    flag[j] = hit;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < Fp; i += blockDim.x) {
    float v = 0.f;
    if (i < F) {
      const int wdw = i / ncep, c = i - wdw * ncep;
      const int ts = t + wdw - ctx;
      if (ts < 0 || ts >= len) v = pad[b];
      else if (!(flag[wdw] | flag[nw + c])) v = centre[((size_t)b * T + ts) * ncep + c];
    }
    dst[i] = v;
  }
}

void launch_expand_context_masked(const float* centre, const float* pad, const int* seq_len, const int* masks, int nm,
                                  int static_width, float* X0, int B, int Bp, int T, int ctx, int ncep, int Fp,
                                  hipStream_t st, int skip) {
  hipLaunchKernelGGL(expand_context_masked_kernel, dim3(skip_frames(T, skip) * Bp), dim3(256), (size_t)(2 * ctx + 1 + ncep), st,
                     centre, pad, seq_len, reinterpret_cast<const int4*>(masks), nm, static_width, X0, B, Bp, T, ctx, ncep, Fp,
                     skip);
}

// ------------------------------------------------------------------ frame skip in a stream session (nasr_stream.hip)
// A feed's new input rows in [S][Tc][F] -> the rows the network sees, out [S][Tk][F], Tk >= every kept[b]: kept row j of
// slot b is input row first[b] + j*skip for j < kept[b] (both worked out on the host from the slot's phase), zeros
// behind them.  Block (j, b) moves one row.
__global__ __launch_bounds__(256) void skip_rows_kernel(const float* __restrict__ in, SkipSlots sk, float* __restrict__ out,
                                                        int Tc, int Tk, int F, int skip) {
  const int j = blockIdx.x, b = blockIdx.y;
  const float* src = j < sk.kept[b] ? in + ((size_t)b * Tc + sk.first[b] + (size_t)j * skip) * F : nullptr;
  float* dst = out + ((size_t)b * Tk + j) * F;
  for (int i = threadIdx.x; i < F; i += blockDim.x) dst[i] = src ? src[i] : 0.f;
}

void launch_skip_rows(const float* in, const SkipSlots& sk, float* out, int S, int Tc, int Tk, int F, int skip, hipStream_t st) {
  hipLaunchKernelGGL(skip_rows_kernel, dim3(Tk, S), dim3(256), 0, st, in, sk, out, Tc, Tk, F, skip);
}

// ------------------------------------------------------------------ look-ahead session (nasr_stream.hip)
// Every slot's window = its held rows, then its new rows; block (t, b) moves pending row t of slot b.  An emitting slot's
// window goes into the chunk's stacked rows win [S][T][F] (zeros behind it, and in the whole of a slot that emits
// nothing: its seq_len is 0), and the rows that stay held, pending rows [emit, P), into the OTHER hold buffer: shifted
// in place they would overlap whenever fewer rows arrive than are held.  win == NULL: no slot emits, the rows only move.
__global__ __launch_bounds__(256) void la_window_kernel(const float* __restrict__ hold_in, const float* __restrict__ fresh,
                                                        LaSlots sl, float* __restrict__ win, float* __restrict__ hold_out,
                                                        int R, int Tc, int T, int F) {
  const int t = blockIdx.x, b = blockIdx.y;
  const int held = sl.held[b], P = held + sl.n[b], E = sl.emit[b];
  const float* src = t < held ? hold_in + ((size_t)b * R + t) * F : t < P ? fresh + ((size_t)b * Tc + (t - held)) * F : nullptr;
  float* wdst = (win && t < T) ? win + ((size_t)b * T + t) * F : nullptr;
  float* hdst = (src && t >= E) ? hold_out + ((size_t)b * R + (t - E)) * F : nullptr;   // t - E < P - E <= R
  for (int i = threadIdx.x; i < F; i += blockDim.x) {
    const float v = src ? src[i] : 0.f;
    if (wdst) wdst[i] = E > 0 ? v : 0.f;
    if (hdst) hdst[i] = v;
  }
}

void launch_la_window(const float* hold_in, const float* fresh, const LaSlots& sl, float* win, float* hold_out, int S, int R,
                      int Tc, int T, int rows, int F, hipStream_t st) {
  hipLaunchKernelGGL(la_window_kernel, dim3(rows, S), dim3(256), 0, st, hold_in, fresh, sl, win, hold_out, R, Tc, T, F);
}

// ------------------------------------------------------------------ latency-controlled training (nasr_pass.hip)
// The windows of every utterance lie one behind the other on a virtual time axis of K windows x W = C + R rows: row
// (k*W + tl)*Bp + b is row tl of window k of utterance b, which is frame k*C + tl.  wlen [K][Bp] = the rows of each window
// (lc_window_rows: 0 behind an utterance's last window and in the padded batch rows).

// src [T*Bp][F] by frame -> dst [K*W*Bp][F] by window row, zeros where a window has no row.  One block per window row.
__global__ __launch_bounds__(256) void lc_gather_kernel(const float* __restrict__ src, const int* __restrict__ wlen,
                                                        float* __restrict__ dst, LcGeom g, int F) {
  const int r = blockIdx.x, b = r % g.Bp, vt = r / g.Bp;
  const int k = vt / g.W, tl = vt - k * g.W;
  const float* sp = tl < wlen[k * g.Bp + b] ? src + ((size_t)(k * g.C + tl) * g.Bp + b) * F : nullptr;
  float* dp = dst + (size_t)r * F;
  for (int i = threadIdx.x; i < F; i += blockDim.x) dp[i] = sp ? sp[i] : 0.f;
}

// The top layer's EMITTED rows by frame: top [T*Bp][DH] <- outv [K*W*Bp][DH]; frame t of utterance b is row t - k*C of
// window k = min(t / C, its last window); zeros from seq_len[b] on.  One block per frame row.
__global__ __launch_bounds__(256) void lc_emit_kernel(const float* __restrict__ outv, const int* __restrict__ seq_len,
                                                      float* __restrict__ top, LcGeom g, int DH) {
  const int r = blockIdx.x, b = r % g.Bp, t = r / g.Bp;
  const int len = seq_len[b];
  const float* sp = nullptr;
  if (t < len) {
    const int k = min(t / g.C, lc_last_window(len, g.C, g.W));
    sp = outv + ((size_t)(k * g.W + t - k * g.C) * g.Bp + b) * DH;
  }
  float* dp = top + (size_t)r * DH;
  for (int i = threadIdx.x; i < DH; i += blockDim.x) dp[i] = sp ? sp[i] : 0.f;
}

// ... and its transpose: the gradient of the top layer's window rows from the gradient by frame.  An emitted row gets its
// frame's gradient, a look-ahead row (tl >= C in a window that is not the utterance's last) and a row no window has get 0.
// Every window row is written by its own block: no sum, no atomics.
__global__ __launch_bounds__(256) void lc_scatter_kernel(const float* __restrict__ dtop, const int* __restrict__ seq_len,
                                                         const int* __restrict__ wlen, float* __restrict__ doutv, LcGeom g,
                                                         int DH) {
  const int r = blockIdx.x, b = r % g.Bp, vt = r / g.Bp;
  const int k = vt / g.W, tl = vt - k * g.W;
  const int P = wlen[k * g.Bp + b];
  const int E = k == lc_last_window(seq_len[b], g.C, g.W) ? P : min(P, g.C);
  const float* sp = tl < E ? dtop + ((size_t)(k * g.C + tl) * g.Bp + b) * DH : nullptr;
  float* dp = doutv + (size_t)r * DH;
  for (int i = threadIdx.x; i < DH; i += blockDim.x) dp[i] = sp ? sp[i] : 0.f;
}

void launch_lc_gather(const float* src, const int* wlen, float* dst, const LcGeom& g, int F, hipStream_t st) {
  hipLaunchKernelGGL(lc_gather_kernel, dim3(g.K * g.W * g.Bp), dim3(256), 0, st, src, wlen, dst, g, F);
}
void launch_lc_emit(const float* outv, const int* seq_len, float* top, const LcGeom& g, int DH, hipStream_t st) {
  hipLaunchKernelGGL(lc_emit_kernel, dim3(g.T * g.Bp), dim3(256), 0, st, outv, seq_len, top, g, DH);
}
void launch_lc_scatter(const float* dtop, const int* seq_len, const int* wlen, float* doutv, const LcGeom& g, int DH,
                       hipStream_t st) {
  hipLaunchKernelGGL(lc_scatter_kernel, dim3(g.K * g.W * g.Bp), dim3(256), 0, st, dtop, seq_len, wlen, doutv, g, DH);
}

}  // namespace nasr
