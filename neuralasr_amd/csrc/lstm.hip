// lstm.hip — the per-timestep LSTM recurrence and its BPTT as gfx950 kernels: the repack of U into their operand images,
// the step and cell kernels, the state a window of steps is carried in from and out to (a stream feed's, a training
// window's), and the two runners that chain the launches of a window (StepWindow, kernels.h).
//
// Semantics (call sites networks/bilstm_ctc_net.py:17-28,
// networks/lstm_ctc_net.py:17-23): g = [x,h]·kernel + bias, gates i,j,f,o,
// c' = c·σ(f+forget_bias) + σ(i)·tanh(j), h' = tanh(c')·σ(o); zero output and carried state past
// seq_len; the bw direction consumes frame seq_len-1-s at step s.  The x·kernel_x + bias half is
// hoisted out of the loop into one MFMA GEMM (gemm.hip); what remains per step is the
// [Bp,Hp]x[Hp,4Hp] recurrent product fused with the cell update.
//
// One launch = one timestep of BOTH directions (blockIdx.y).  Measured on MI355X (with a per-step microbenchmark since removed):
// a dependent launch costs 1.55 us whatever its shape, and a CU pulls only ~35-70 GB/s from the Infinity
// Cache / its XCD's L2 (PMC: every launch re-fetches the matrices through the fabric, the L2s do not keep
// them across a kernel boundary), so a step is priced by BYTES PER CU, not by chip bandwidth.  Both kernels
// are therefore cut so that every CU streams ~32 KB of recurrent weights plus the smallest possible share
// of the step's state:
//   forward : block = 4 hidden units x 4 gates (one 16-column MFMA tile), Hp/4 * D blocks (256 for
//             2x512), its 4 waves split K = Hp and reduce through LDS; state = h (32 KB).
//   backward: block = (64-unit output tile, 32-unit K slice); it rebuilds its slice of dG from the
//             previous launch's partial sums, multiplies by its 32 KB tile of U^T and hands 16 x 64
//             partial sums to the next launch (split-K across launches: deterministic, no atomics).
// Operands are stored in HBM in MFMA-fragment order ("swizzled"), four k-steps per 16-byte load, so
// every wave load is one contiguous 1 KiB.
//
// MFMA 16x16x4 f32 fragment maps: A[row = l&15][k = l>>4], B[k = l>>4][col = l&15],
// C/D col = l&15, row = 4*(l>>4) + reg.
#include "kernels.h"
#include "lstm_device.h"

namespace nasr {

// Element (row b16, unit k) of M-tile mt inside the swizzled h-state image (contraction length Kd).
// Lane l of 16-byte group q holds, in component i, the value the MFMA k-step 4q+i wants from lane l:
// unit k = 16q + 4*(l>>4) + i, row l&15.  The 4 units x 16 rows one block produces are therefore one
// contiguous 256-byte run (coalesced state write).
__device__ __forceinline__ int sw_index(int Kd, int mt, int b16, int k) {
  return ((((mt * (Kd >> 4) + (k >> 4)) * 64) + ((k >> 2) & 3) * 16 + b16) << 2) + (k & 3);
}

// ------------------------------------------------------------------ recurrent weight repack
// U [Hp][N4] (row k = h unit, col n = 4*j+g) ->
//   Uf [N4/16 tiles][Hp/16][64][4] : Uf[tile][q][l][i] = U[16q + 4*(l>>4) + i][16*tile + (l&15)]
//        forward B operand; k-step 4q+i contracts units {16q + 4*sub + i}, matching sw_index().
//   Ub [Hp/64 jt][Hp/32 ks][4 w][4 nt][2 q2][64][4] :
//        Ub[..][l][i] = U[64jt + 16nt + (l&15)][4*(32ks + 4*(4q2+i) + (l>>4)) + w]
//        backward B operand (= U^T): block (jt,ks), wave w = gate w, k-step 4q2+i contracts the
//        slice-local units {4*(4q2+i) + sub}.
__global__ __launch_bounds__(256) void repack_u_kernel(const float* __restrict__ U, float* __restrict__ Uf,
                                                       float* __restrict__ Ub, int Hp) {
  const int N4 = 4 * Hp;
  const int64_t total = (int64_t)Hp * N4;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int i = e & 3, l = (e >> 2) & 63;
    {  // forward image
      const int64_t tq = e >> 8;
      const int q = (int)(tq % (Hp >> 4)), tile = (int)(tq / (Hp >> 4));
      Uf[e] = U[(size_t)(16 * q + 4 * (l >> 4) + i) * N4 + 16 * tile + (l & 15)];
    }
    {  // backward image
      int64_t x = e >> 8;
      const int q2 = (int)(x & 1); x >>= 1;
      const int nt = (int)(x & 3); x >>= 2;
      const int w = (int)(x & 3); x >>= 2;
      const int ks = (int)(x % (Hp >> 5)), jt = (int)(x / (Hp >> 5));
      const int ju = 4 * (4 * q2 + i) + (l >> 4);
      Ub[e] = U[(size_t)(64 * jt + 16 * nt + (l & 15)) * N4 + 4 * (32 * ks + ju) + w];
    }
  }
}

void launch_repack_u(const float* U, float* Uf, float* Ub, int Hp, hipStream_t st) {
  hipLaunchKernelGGL(repack_u_kernel, dim3(1024), dim3(256), 0, st, U, Uf, Ub, Hp);
}

// ------------------------------------------------------------------ forward step
// NQ = Hp/64 (16-byte operand groups per wave) as a template constant keeps the load/MFMA stream
// straight-line, so hipcc emits counted vmcnt waits and the MFMA chain starts when the first pair lands;
// NQ = 0 is the generic (runtime) form.
// CARRY: the state-carrying form of a stream feed (nasr_stream.hip).  Step 0 continues a sequence instead of starting
// one: hin is the saved h, written in the layout of sw_index by load_carry_kernel, and c_{-1} is c0 [D][Bp][Hp]
// instead of 0.  Everything else, and every step s > 0, is the batch form, which never reads c0.
template <int MT, int NQ, bool CARRY = false>
__global__ __launch_bounds__(256) void lstm_fwd_step_kernel(
    const float* __restrict__ Uf,    // [D][Hp/4][Hp/16][64][4]
    const float* __restrict__ hin,   // [D][MT][Hp/16][64][4]
    float* __restrict__ hout, float* __restrict__ gates, float* __restrict__ cbuf, float* __restrict__ out,
    const int* __restrict__ seq_len, int s, int T, int Bp, int Hp, int D, float fb, const float* __restrict__ c0) {
  __shared__ __attribute__((aligned(16))) float red[4][MT][64][4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int tile = blockIdx.x, d = blockIdx.y;
  const int N4 = 4 * Hp, DH = D * Hp, DN = D * N4;
  const int nq = NQ > 0 ? NQ : (Hp >> 6);   // float4 groups per wave (K quarter)
  const int q0 = w * nq;
  constexpr int CH = NQ == 0 ? 1 : (NQ < 8 ? NQ : 8);

  // seq_len first: vmcnt retires in order, so the wait on it must not sit behind the operand stream
  const int cmt = tid >> 6, cl = tid & 63;
  const int b16 = cl & 15, u = cl >> 4;
  const int b = cmt * 16 + b16;
  const int len_ld = seq_len[b < Bp ? b : 0];

  // ---- recurrent product: acc[mt] (16 x 16) over this wave's K quarter.  Loads are issued in
  // consumption order (h, U, h, U, ...) ahead of everything else.
  const float4* ub = reinterpret_cast<const float4*>(Uf) + ((size_t)(d * (Hp >> 2) + tile) * (Hp >> 4) + q0) * 64 + lane;
  const float4* ha = reinterpret_cast<const float4*>(hin) + ((size_t)d * MT * (Hp >> 4) + q0) * 64 + lane;
  float4 bu[CH];
  float4 av[MT][CH];
  // (the h operands of the first chunk are loaded as temporaries: a plain assignment gives hipcc a different schedule)
#pragma unroll
  for (int x = 0; x < CH; ++x) {
#pragma unroll
    for (int m = 0; m < MT; ++m)
      av[m][x] = float4(ha[((size_t)m * (Hp >> 4) + x) * 64]);
    bu[x] = ub[(size_t)x * 64];
  }

  // ---- cell threads: issue the loads the cell update needs
  const bool cell = tid < 64 * MT;
  const int j = tile * 4 + u;
  int len = 0;
  bool valid = false;
  int r = 0;
  float4 xg = make_float4(0.f, 0.f, 0.f, 0.f);
  float cprev = 0.f;
  if (cell) {
    len = len_ld;
    valid = s < len;
    if (valid) {
      const int tb = d ? (len - 1 - s) : s;
      r = tb * Bp + b;
      xg = *reinterpret_cast<const float4*>(gates + (size_t)r * DN + d * N4 + 4 * j);
      if (s > 0) cprev = cbuf[(size_t)(d ? r + Bp : r - Bp) * DH + d * Hp + j];
      else if (CARRY) cprev = c0[((size_t)d * Bp + b) * Hp + j];
    }
  }

  f32x4 acc[MT][2];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    acc[m][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
    acc[m][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  for (int qc = 0; qc < nq; qc += CH) {
    if (qc > 0) {
#pragma unroll
      for (int x = 0; x < CH; ++x) {
#pragma unroll
        for (int m = 0; m < MT; ++m)
          av[m][x] = ha[((size_t)m * (Hp >> 4) + qc + x) * 64];
        bu[x] = ub[(size_t)(qc + x) * 64];
      }
    }
#pragma unroll
    for (int x = 0; x < CH; ++x) {
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        acc[m][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m][x].x, bu[x].x, acc[m][0], 0, 0, 0);
        acc[m][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m][x].y, bu[x].y, acc[m][1], 0, 0, 0);
        acc[m][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m][x].z, bu[x].z, acc[m][0], 0, 0, 0);
        acc[m][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m][x].w, bu[x].w, acc[m][1], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    f32x4 sacc = acc[m][0] + acc[m][1];
    *reinterpret_cast<f32x4*>(&red[w][m][lane][0]) = sacc;
  }
  __syncthreads();

  // ---- fused cell update: thread = (batch row b, hidden unit j)
  if (cell) {
    float* hdst = hout + (size_t)d * MT * Hp * 16 + sw_index(Hp, cmt, b16, j);
    if (valid) {
      const int ls = 16 * (b16 >> 2) + 4 * u, rg = b16 & 3;
      float g[4];
#pragma unroll
      for (int gi = 0; gi < 4; ++gi)
        g[gi] = red[0][cmt][ls + gi][rg] + red[1][cmt][ls + gi][rg] + red[2][cmt][ls + gi][rg] + red[3][cmt][ls + gi][rg];
      const f32x4 act = lstm_gates((f32x4){xg.x + g[0], xg.y + g[1], xg.z + g[2], xg.w + g[3]}, fb);
      float c = cprev;
      const float h = lstm_state(act, c);
      *reinterpret_cast<float4*>(gates + (size_t)r * DN + d * N4 + 4 * j) = to_float4(act);
      cbuf[(size_t)r * DH + d * Hp + j] = c;
      out[(size_t)r * DH + d * Hp + j] = h;
      *hdst = h;
    } else {
      // frame s of row b is past seq_len for both directions: zero output (A.2); state is dead
      if (s < T) out[((size_t)s * Bp + b) * DH + d * Hp + j] = 0.f;
      *hdst = 0.f;
    }
  }
}

using StepMT = std::integer_sequence<int, 1, 2, 3, 4>;   // MT = Bp/16 M tiles of the step kernels

// c0 == NULL: step s of a sequence; c0 != NULL (s = 0): the first step of a stream feed or of a training window, from
// hin = the carried h as an operand image and c0 = the carried c [D][Bp][Hp]
static void fwd_step(const LstmDims& dm, int s, const float* Uf, const float* hin, float* hout, float* gates, float* cbuf,
                     float* out, const int* seq_len, float forget_bias, const float* c0, hipStream_t st) {
  dim3 grid(dm.Hp / 4, dm.D), block(256);
  dispatch_int(StepMT{}, dm.Bp / 16, [&](auto mt) {
    dispatch_int(std::integer_sequence<int, 1, 2, 4, 8, 16, 0>{}, dm.Hp / 64, [&](auto nq) {   // NQ = Hp/64, 0 = the generic form
      if (c0)
        hipLaunchKernelGGL((lstm_fwd_step_kernel<mt(), nq(), true>), grid, block, 0, st, Uf, hin, hout, gates, cbuf, out, seq_len,
                           0, dm.T, dm.Bp, dm.Hp, dm.D, forget_bias, c0);
      else
        hipLaunchKernelGGL((lstm_fwd_step_kernel<mt(), nq()>), grid, block, 0, st, Uf, hin, hout, gates, cbuf, out, seq_len, s,
                           dm.T, dm.Bp, dm.Hp, dm.D, forget_bias, static_cast<const float*>(nullptr));
    });
  });
}

// ------------------------------------------------------------------ carried state (nasr_stream.hip; nasr_pass.hip)
// What step 0 of a stream feed or of a training window reads, for every direction (blockIdx.y): the h operand image
// [Bp/16][Hp/16][64][4] in the layout of sw_index and c [Bp][Hp].  Direction 0 comes from the source: row b's c and h are
// `units` floats at c / h + b * stride, for the rows b < rows with live[b] > 0 (live == NULL: all of them).  A backward
// direction starts every window anew, from zeros; padded units and every other row: zeros.  Every element of both images is
// written on every launch.
struct CarrySrc { const float *c, *h; int stride, rows, units; const int* live; };
__global__ __launch_bounds__(256) void load_carry_kernel(CarrySrc src, float* __restrict__ himg, float* __restrict__ cimg, int Bp,
                                                         int Hp) {
  const int e = blockIdx.x * 256 + threadIdx.x, d = blockIdx.y;
  if (e >= Bp * Hp) return;
  const int b = e / Hp, j = e - b * Hp;
  float c = 0.f, hv = 0.f;
  if (d == 0 && b < src.rows && j < src.units && (!src.live || src.live[b] > 0)) {
    c = src.c[(size_t)b * src.stride + j];
    hv = src.h[(size_t)b * src.stride + j];
  }
  cimg[(size_t)d * Bp * Hp + e] = c;
  himg[(size_t)d * Bp * Hp + sw_index(Hp, b >> 4, b & 15, j)] = hv;
}
static void load_carry(const CarrySrc& src, float* himg, float* cimg, int Bp, int Hp, int D, hipStream_t st) {
  hipLaunchKernelGGL(load_carry_kernel, dim3((Bp * Hp + 255) / 256, D), dim3(256), 0, st, src, himg, cimg, Bp, Hp);
}

// a stream session's saved forward state of one layer, natural layout [S][2][H] (c, then h): slots b < S, units j < H
void launch_stream_load_state(const float* state, float* himg, float* cimg, int S, int H, int Bp, int Hp, hipStream_t st, int D) {
  load_carry({state, state + H, 2 * H, S, H, nullptr}, himg, cimg, Bp, Hp, D, st);
}
// window k of a chunked batch continues from row C-1 of window k-1 of this layer's out / cbuf [K*W*Bp][DH] (the state after
// the last row that window emitted), for the utterances with rows in window k; nothing is live for window 0
void launch_lc_load_carry(const float* out, const float* cbuf, const int* wlen, int k, const LcGeom& g, float* himg, float* cimg,
                          int Hp, int D, hipStream_t st) {
  const size_t r = k > 0 ? (size_t)((k - 1) * g.W + g.C - 1) * g.Bp * D * Hp : 0;
  load_carry({cbuf + r, out + r, D * Hp, k > 0 ? g.Bp : 0, Hp, wlen + (size_t)k * g.Bp}, himg, cimg, g.Bp, Hp, D, st);
}

// ... and back into a stream session's state [S][2][H]: the forward direction's (c, h) after every slot's last EMITTED row,
// the first Hp of row (emit[b] - 1) * Bp + b of cbuf / out [T * Bp][DH]; the look-ahead rows behind it are run again by the
// next window.  A slot that emits nothing keeps what it had.
__global__ __launch_bounds__(256) void stream_save_state_kernel(const float* __restrict__ out, const float* __restrict__ cbuf,
                                                                LaSlots sl, float* __restrict__ state, int S, int H, int Bp, int DH) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= S * H) return;
  const int b = e / H, j = e - b * H;
  const int E = sl.emit[b];
  if (E < 1) return;
  const size_t r = (size_t)(E - 1) * Bp + b;
  state[((size_t)b * 2 + 0) * H + j] = cbuf[r * DH + j];
  state[((size_t)b * 2 + 1) * H + j] = out[r * DH + j];
}

void launch_stream_save_state(const float* out, const float* cbuf, const LaSlots& sl, float* state, int S, int H, int Bp, int DH,
                              hipStream_t st) {
  hipLaunchKernelGGL(stream_save_state_kernel, dim3((S * H + 255) / 256), dim3(256), 0, st, out, cbuf, sl, state, S, H, Bp, DH);
}

// ------------------------------------------------------------------ BPTT step
// grid.x = (Hp/64 output tiles jt) x (Hp/32 K slices ks), blockIdx.x = jt*KSPLIT + ks so the blocks that
// rebuild the same dG slice share an XCD (ids equal mod 8).  Per block and step:
//   P: for its 32 units x Bp rows: dh = sum_k partial_in[k] + dOut (gradient from above), gate
//      derivatives from the saved activations -> dG slice [Bp x 128] into LDS (k order g*32+ju);
//      the jt == 0 block also stores dG frame-indexed (for the weight-gradient GEMMs) and dc.
//   G: partial_out[ks][b][64jt..] = dG_slice x U^T tile on v_mfma_f32_16x16x4 (wave w = gate w),
//      4-wave LDS reduction, plain stores.  The next launch sums the KSPLIT partials in fixed order.
// Masked frames get dG = 0 so the GEMMs need no mask.
// Wide layers (Hp > 512, e.g. DeepSpeech's 2048): every output tile's block would re-sum the same Hp/32 partials
// (Hp^3 traffic: 434 us per step at Hp = 2048).  There the step is two launches: lstm_bwd_cell_kernel sums the partials
// and does the cell arithmetic ONCE per cell (writing dG frame-indexed), and this kernel runs with PRE = true: its P
// stage only copies its dG slice from that buffer, and each block walks KSL = 4 consecutive K slices with the
// accumulators kept in registers, so 4x fewer partial sums are handed on.
// CARRY: the counterpart of lstm_fwd_step_kernel<.., CARRY> for a window of latency-controlled training,
// launched for step 0 only.  The forward step started from the carried c0 [D][Bp][Hp] (zeros for a backward direction)
// instead of 0, so the forget gate's derivative reads it.  Nothing else differs: dcout is dc . f and the partial sums are
// dG x U^T at every step, which after step 0 are the gradients with respect to the carried (c, h).
template <int MT, int KSP, bool PRE = false, int KSL = 1, bool CARRY = false>
__global__ __launch_bounds__(256) void lstm_bwd_step_kernel(
    const float* __restrict__ Ub,     // [D][Hp/64][Hp/32][4][4][2][64][4]
    const float* __restrict__ pin,    // [D][KSPLIT][Bp][Hp] partial sums of dh_rec from the previous launch
    float* __restrict__ pout,
    const float* __restrict__ gates,  // [R][D*N4] activations si,tj,sf,so
    float* __restrict__ dgbuf,        // [R][D*N4] dG, frame indexed
    const float* __restrict__ cbuf, const float* __restrict__ dout, const float* __restrict__ dcin,
    float* __restrict__ dcout, const int* __restrict__ seq_len, int s, int T, int Bp, int Hp, int D,
    const float* __restrict__ c0) {
  // wide form (PRE): the reduction buffer reuses the dG slice's LDS (32 KB instead of 49 KB at MT = 2), so that the four
  // blocks a CU gets at Hp = 2048 are resident together instead of three and a straggler
  constexpr int AS_FLOATS = MT * 128 * 17, RED_FLOATS = 4 * MT * 4 * 64 * 4;
  __shared__ __attribute__((aligned(16))) float lds_[PRE ? (AS_FLOATS > RED_FLOATS ? AS_FLOATS : RED_FLOATS) : AS_FLOATS + RED_FLOATS];
  float (*As)[128][17] = reinterpret_cast<float (*)[128][17]>(lds_);
  float (*red)[MT][4][64][4] = reinterpret_cast<float (*)[MT][4][64][4]>(PRE ? lds_ : lds_ + AS_FLOATS);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int KSPLIT = KSP > 0 ? KSP : (Hp >> 5);     // K slices of 32 units in the operand image
  const int NKG = KSPLIT / KSL;                      // K-slice groups = partial sums per output
  const int jt = blockIdx.x / NKG, ksg = blockIdx.x % NKG, d = blockIdx.y;
  const int N4 = 4 * Hp, DH = D * Hp, DN = D * N4;
  f32x4 acc[MT][4];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[m][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int kl = 0; kl < KSL; ++kl) {
  const int ks = ksg * KSL + kl;
  if (KSL > 1 && kl > 0) __syncthreads();            // the previous slice's fragment reads of As are done
  // ---- this wave's 8 B-operand fragments (32 KB per block), in flight during the P stage
  const float4* ub = reinterpret_cast<const float4*>(Ub) +
                     ((((size_t)(d * (Hp >> 6) + jt) * KSPLIT + ks) * 4 + w) * 8) * 64 + lane;
  float4 bu[4][2];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int q2 = 0; q2 < 2; ++q2) bu[nt][q2] = ub[(size_t)(nt * 2 + q2) * 64];

  // ---- P stage: 2*MT cells per thread, processed in pairs: every load of a pair is issued before any
  // of its arithmetic so the two latency chains overlap.
  const float* pbase = pin + (size_t)d * KSPLIT * Bp * Hp;
  constexpr int KV = KSP > 0 ? KSP : 1;
  if constexpr (PRE) {
#pragma unroll
    for (int cp = 0; cp < 2 * MT; ++cp) {
      const int c = tid + 256 * cp;
      const int ju = c & 31, b = c >> 5;
      const int mt = b >> 4, b16 = b & 15;
      const int len = seq_len[b];
      const int tb = s < len ? (d ? (len - 1 - s) : s) : s;
      const float4 dg = *reinterpret_cast<const float4*>(dgbuf + ((size_t)tb * Bp + b) * DN + d * N4 + 4 * (32 * ks + ju));
      As[mt][0 * 32 + ju][b16] = dg.x;
      As[mt][1 * 32 + ju][b16] = dg.y;
      As[mt][2 * 32 + ju][b16] = dg.z;
      As[mt][3 * 32 + ju][b16] = dg.w;
    }
  } else {
#pragma unroll
  for (int cp2 = 0; cp2 < MT; ++cp2) {
    int lenv[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) lenv[e] = seq_len[(tid + 256 * (2 * cp2 + e)) >> 5];
    float4 a[2];
    float cc[2], cpv[2], dh[2], dci[2], pv[2][KV];
    int rr[2];
    bool val[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int c = tid + 256 * (2 * cp2 + e);
      const int ju = c & 31, b = c >> 5;
      const int j = 32 * ks + ju;
      val[e] = s < lenv[e];
      const int tb = val[e] ? (d ? (lenv[e] - 1 - s) : s) : 0;
      const int r = tb * Bp + b;
      rr[e] = r;
      // unconditional loads (a masked cell reads frame 0 of its row and is zeroed below): no divergent
      // branch, so both cells' loads are in flight together
      const int rp = s > 0 ? (d ? r + Bp : r - Bp) : r;
      a[e] = *reinterpret_cast<const float4*>(gates + (size_t)r * DN + d * N4 + 4 * j);  // si,tj,sf,so
      cc[e] = cbuf[(size_t)r * DH + d * Hp + j];
      if constexpr (CARRY) cpv[e] = c0[((size_t)d * Bp + b) * Hp + j];
      else cpv[e] = cbuf[(size_t)(val[e] ? rp : r) * DH + d * Hp + j];
      dh[e] = dout[(size_t)r * DH + d * Hp + j];
      dci[e] = dcin[((size_t)d * Bp + b) * Hp + j];
      const float* pp = pbase + (size_t)b * Hp + j;
      if (KSP > 0) {
#pragma unroll
        for (int k = 0; k < KV; ++k) pv[e][k] = pp[(size_t)k * Bp * Hp];
      } else {
        float acc0 = 0.f;
        for (int k = 0; k < KSPLIT; ++k) acc0 += pp[(size_t)k * Bp * Hp];
        pv[e][0] = acc0;
      }
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int c = tid + 256 * (2 * cp2 + e);
      const int ju = c & 31, b = c >> 5;
      const int mt = b >> 4, b16 = b & 15;
      const int j = 32 * ks + ju;
      float4 dg = make_float4(0.f, 0.f, 0.f, 0.f);
      float dcn = 0.f;
      if (val[e]) {
        float dhs = dh[e];
#pragma unroll
        for (int k = 0; k < KV; ++k) dhs += pv[e][k];
        dg = to_float4(lstm_cell_bwd(to_f32x4(a[e]), cc[e], cpv[e], !CARRY && s == 0, dhs, dci[e], dcn));
      }
      if (jt == 0) {   // the frame of a masked step is frame s itself (past seq_len in both directions): dG = 0 there
        const size_t row = val[e] ? (size_t)rr[e] : (size_t)s * Bp + b;
        *reinterpret_cast<float4*>(dgbuf + row * DN + d * N4 + 4 * j) = dg;
        dcout[((size_t)d * Bp + b) * Hp + j] = dcn;
      }
      As[mt][0 * 32 + ju][b16] = dg.x;
      As[mt][1 * 32 + ju][b16] = dg.y;
      As[mt][2 * 32 + ju][b16] = dg.z;
      As[mt][3 * 32 + ju][b16] = dg.w;
    }
  }
  }   // !PRE
  __syncthreads();

  // ---- G stage: wave w contracts k_local in [32w, 32w+32) (gate w) for the 4 N-tiles
#pragma unroll
  for (int q2 = 0; q2 < 2; ++q2) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int kl = 32 * w + 4 * (4 * q2 + i) + (lane >> 4);
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const float a = As[m][kl][lane & 15];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const float bv = i == 0 ? bu[nt][q2].x : i == 1 ? bu[nt][q2].y : i == 2 ? bu[nt][q2].z : bu[nt][q2].w;
          acc[m][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc[m][nt], 0, 0, 0);
        }
      }
    }
  }
  }   // K-slice loop
  if (PRE) __syncthreads();                            // every wave's fragment reads of As are done: red overwrites it
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) *reinterpret_cast<f32x4*>(&red[w][m][nt][lane][0]) = acc[m][nt];
  __syncthreads();

  // ---- wave w finalises N-tile w: C/D map col = lane&15 (unit), row = 4*(lane>>4)+reg (batch row)
  float* po = pout + ((size_t)d * NKG + ksg) * Bp * Hp;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(&red[0][m][w][lane][0]) +
                    *reinterpret_cast<const f32x4*>(&red[1][m][w][lane][0]) +
                    *reinterpret_cast<const f32x4*>(&red[2][m][w][lane][0]) +
                    *reinterpret_cast<const f32x4*>(&red[3][m][w][lane][0]);
    const int jo = 64 * jt + 16 * w + (lane & 15);
    const int b0 = 16 * m + 4 * (lane >> 4);
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {   // (address before value: the other order gives hipcc a different schedule)
      float* p = &po[(size_t)(b0 + rg) * Hp + jo];
      *p = v[rg];
    }
  }
}

// one thread per cell (b, j) of direction d: dh = sum of the NP partial sums + dOut, gate derivatives, dc; writes the
// frame-indexed dG row (zero at masked frames) and the carried dc
__global__ __launch_bounds__(256) void lstm_bwd_cell_kernel(const float* __restrict__ pin, int NP,
                                                            const float* __restrict__ gates, float* __restrict__ dgbuf,
                                                            const float* __restrict__ cbuf, const float* __restrict__ dout,
                                                            const float* __restrict__ dcin, float* __restrict__ dcout,
                                                            const int* __restrict__ seq_len, int s, int Bp, int Hp, int D) {
  const int c = blockIdx.x * 256 + threadIdx.x, d = blockIdx.y;
  if (c >= Bp * Hp) return;
  const int j = c % Hp, b = c / Hp;
  const int N4 = 4 * Hp, DH = D * Hp, DN = D * N4;
  const int len = seq_len[b];
  const bool val = s < len;
  const int tb = val ? (d ? (len - 1 - s) : s) : s;
  const size_t r = (size_t)tb * Bp + b;
  float4 dg = make_float4(0.f, 0.f, 0.f, 0.f);
  float dcn = 0.f;
  if (val) {
    const float* pp = pin + (size_t)d * NP * Bp * Hp + (size_t)b * Hp + j;
    float dhs = dout[r * DH + d * Hp + j];
    float s0 = 0.f, s1 = 0.f;
    int k = 0;
    for (; k + 1 < NP; k += 2) { s0 += pp[(size_t)k * Bp * Hp]; s1 += pp[(size_t)(k + 1) * Bp * Hp]; }
    if (k < NP) s0 += pp[(size_t)k * Bp * Hp];
    dhs += s0 + s1;
    const float4 a = *reinterpret_cast<const float4*>(gates + r * DN + d * N4 + 4 * j);
    const float cc = cbuf[r * DH + d * Hp + j];
    const float cpv = s > 0 ? cbuf[(d ? r + Bp : r - Bp) * DH + d * Hp + j] : 0.f;   // (no frame before the first one to read)
    dg = to_float4(lstm_cell_bwd(to_f32x4(a), cc, cpv, s == 0, dhs, dcin[((size_t)d * Bp + b) * Hp + j], dcn));
  }
  *reinterpret_cast<float4*>(dgbuf + r * DN + d * N4 + 4 * j) = dg;
  dcout[((size_t)d * Bp + b) * Hp + j] = dcn;
}

// The same for step 0 of a window whose forward step started from the carried c0 [D][Bp][Hp] (the CARRY form of
// lstm_bwd_step_kernel).  A kernel of its own: sharing the body changes the instruction schedule of the one above.
__global__ __launch_bounds__(256) void lstm_bwd_cell_carry_kernel(const float* __restrict__ pin, int NP,
                                                                  const float* __restrict__ gates, float* __restrict__ dgbuf,
                                                                  const float* __restrict__ cbuf, const float* __restrict__ dout,
                                                                  const float* __restrict__ dcin, float* __restrict__ dcout,
                                                                  const int* __restrict__ seq_len, int Bp, int Hp, int D,
                                                                  const float* __restrict__ c0) {
  const int c = blockIdx.x * 256 + threadIdx.x, d = blockIdx.y;
  if (c >= Bp * Hp) return;
  const int j = c % Hp, b = c / Hp;
  const int N4 = 4 * Hp, DH = D * Hp, DN = D * N4;
  const int len = seq_len[b];
  const bool val = len > 0;
  const size_t r = (size_t)(val && d ? len - 1 : 0) * Bp + b;
  float4 dg = make_float4(0.f, 0.f, 0.f, 0.f);
  float dcn = 0.f;
  if (val) {
    const float* pp = pin + (size_t)d * NP * Bp * Hp + (size_t)b * Hp + j;
    float dhs = dout[r * DH + d * Hp + j];
    float s0 = 0.f, s1 = 0.f;
    int k = 0;
    for (; k + 1 < NP; k += 2) { s0 += pp[(size_t)k * Bp * Hp]; s1 += pp[(size_t)(k + 1) * Bp * Hp]; }
    if (k < NP) s0 += pp[(size_t)k * Bp * Hp];
    dhs += s0 + s1;
    const float4 a = *reinterpret_cast<const float4*>(gates + r * DN + d * N4 + 4 * j);
    dg = to_float4(lstm_cell_bwd(to_f32x4(a), cbuf[r * DH + d * Hp + j], c0[((size_t)d * Bp + b) * Hp + j], false, dhs,
                                 dcin[((size_t)d * Bp + b) * Hp + j], dcn));
  }
  *reinterpret_cast<float4*>(dgbuf + r * DN + d * N4 + 4 * j) = dg;
  dcout[((size_t)d * Bp + b) * Hp + j] = dcn;
}

// partial sums a BPTT step hands on: Hp/32 of them per output, Hp/128 for the wide-layer form
constexpr int BWD_KSL = 4;   // K slices a block of the wide form walks (A/B: 2, 4, 8)
static bool bwd_wide_form(int Hp) { return Hp > 512 && Hp % (32 * BWD_KSL) == 0; }
int lstm_bwd_partials(int Hp) { return bwd_wide_form(Hp) ? Hp / (32 * BWD_KSL) : Hp / 32; }

// c0 == NULL: step s of a sequence; c0 != NULL (s = 0): step 0 of a window that continued from the carried c0
static void bwd_step(const LstmDims& dm, int s, const float* Ub, const float* pin, float* pout, const float* gates, float* dgbuf,
                     const float* cbuf, const float* dout, const float* dcin, float* dcout, const int* seq_len, const float* c0,
                     hipStream_t st) {
  if (bwd_wide_form(dm.Hp)) {     // wide layer: cell arithmetic once, then the product (see the kernel's header)
    const int np = dm.Hp / (32 * BWD_KSL);
    const dim3 gridc((dm.Bp * dm.Hp + 255) / 256, dm.D);
    if (c0)
      hipLaunchKernelGGL(lstm_bwd_cell_carry_kernel, gridc, dim3(256), 0, st, pin, np, gates, dgbuf, cbuf, dout, dcin, dcout,
                         seq_len, dm.Bp, dm.Hp, dm.D, c0);
    else
      hipLaunchKernelGGL(lstm_bwd_cell_kernel, gridc, dim3(256), 0, st, pin, np, gates, dgbuf, cbuf, dout, dcin, dcout, seq_len, s,
                         dm.Bp, dm.Hp, dm.D);
    dim3 gridw((dm.Hp / 64) * np, dm.D);
    dispatch_int(StepMT{}, dm.Bp / 16, [&](auto mt) {
      hipLaunchKernelGGL((lstm_bwd_step_kernel<mt(), 0, true, BWD_KSL>), gridw, dim3(256), 0, st, Ub, pin, pout, gates, dgbuf,
                         cbuf, dout, dcin, dcout, seq_len, s, dm.T, dm.Bp, dm.Hp, dm.D, static_cast<const float*>(nullptr));
    });
    return;
  }
  dim3 grid((dm.Hp / 64) * (dm.Hp / 32), dm.D), block(256);
  dispatch_int(StepMT{}, dm.Bp / 16, [&](auto mt) {
    dispatch_int(std::integer_sequence<int, 2, 4, 8, 16, 0>{}, dm.Hp / 32, [&](auto ksp) {   // KSP = Hp/32, 0 = the generic form
      if (c0)
        hipLaunchKernelGGL((lstm_bwd_step_kernel<mt(), ksp(), false, 1, true>), grid, block, 0, st, Ub, pin, pout, gates, dgbuf,
                           cbuf, dout, dcin, dcout, seq_len, 0, dm.T, dm.Bp, dm.Hp, dm.D, c0);
      else
        hipLaunchKernelGGL((lstm_bwd_step_kernel<mt(), ksp()>), grid, block, 0, st, Ub, pin, pout, gates, dgbuf, cbuf, dout,
                           dcin, dcout, seq_len, s, dm.T, dm.Bp, dm.Hp, dm.D, static_cast<const float*>(nullptr));
    });
  });
}

// ------------------------------------------------------------------ a window of steps (StepWindow, kernels.h)
// How the per-step launches chain, here and nowhere else: forward step s reads h image s & 1 and writes the other; BPTT
// step s, the (T-1-s)-th of its chain, reads that parity's partial-sum and dc images and writes the other.
static size_t h_image(const StepWindow& w) { return (size_t)w.dm.D * w.dm.Bp * w.dm.Hp; }
static size_t p_image(const StepWindow& w) { return h_image(w) * lstm_bwd_partials(w.dm.Hp); }

float* lstm_steps_dcin(const StepWindow& w, int s) { return w.dcstate + ((w.dm.T - 1 - s) & 1) * h_image(w); }
StepLeft lstm_steps_left(const StepWindow& w, int s) {
  const int wr = (w.dm.T - s) & 1;
  return {w.partial + wr * p_image(w), w.dcstate + wr * h_image(w)};
}

void lstm_steps_fwd(const StepWindow& w, int s0, int s1, hipStream_t st) {
  const size_t hs = h_image(w);
  if (s0 == 0 && s1 > 0 && !w.c0) (void)hipMemsetAsync(w.hstate, 0, hs * 4, st);
  for (int s = s0; s < s1; ++s)
    fwd_step(w.dm, s, w.Uf, w.hstate + (s & 1) * hs, w.hstate + ((s + 1) & 1) * hs, w.gates, w.cbuf, w.out, w.seq_len,
             w.forget_bias, s == 0 ? w.c0 : nullptr, st);
}

void lstm_steps_bwd(const StepWindow& w, int s0, int s1, hipStream_t st) {
  if (s1 == w.dm.T && s0 < s1) {   // the chain starts here: once per window, however its steps are cut into ranges
    (void)hipMemsetAsync(w.partial, 0, p_image(w) * 4, st);
    (void)hipMemsetAsync(w.dcstate, 0, h_image(w) * 4, st);
  }
  for (int s = s1 - 1; s >= s0; --s) {
    const StepLeft o = lstm_steps_left(w, s);
    bwd_step(w.dm, s, w.Ub, lstm_steps_left(w, s + 1).partial, o.partial, w.gates, w.dg, w.cbuf, w.dout, lstm_steps_dcin(w, s),
             o.dc, w.seq_len, s == 0 ? w.c0 : nullptr, st);
  }
}

// ------------------------------------------------------------------ latency-controlled training (nasr_pass.hip)
// The windows of every utterance lie one behind the other on a virtual time axis of K windows x W = C + R rows (rows.hip
// moves the rows there and back); wlen [K][Bp] = the rows of each window.  Here: what crosses a window boundary in BPTT.

// Behind step 0 of window k's BPTT (k >= 1): the gradient with respect to the forward direction's carried (h, c) goes to
// where the state came from.  dh = the NP partial sums that launch left (direction 0: the head of `part`), summed in their
// order, is ADDED to the forward half of window k-1's row C-1 of dout (drow = that row, [Bp][DH]); dc = its dcout is kept
// in dcc [Bp][Hp] until window k-1's BPTT reaches that step (lc_carry_dc_kernel).  An utterance without rows in window k
// hands back zeros.  One thread per (b, j): one writer, fixed order.
__global__ __launch_bounds__(256) void lc_carry_out_kernel(const float* __restrict__ part, int NP, const float* __restrict__ dcs,
                                                           const int* __restrict__ wlen_k, float* __restrict__ drow,
                                                           float* __restrict__ dcc, int Bp, int Hp, int DH) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= Bp * Hp) return;
  const int b = e / Hp, j = e - b * Hp;
  float dc = 0.f;
  if (wlen_k[b] > 0) {
    float dh = 0.f;
    for (int p = 0; p < NP; ++p) dh += part[(size_t)p * Bp * Hp + e];
    drow[(size_t)b * DH + j] += dh;
    dc = dcs[e];
  }
  dcc[e] = dc;
}

// ... dc joins the chain: dcin [Bp][Hp] is what the forward direction's BPTT step C-1 of window k-1 is about to read
__global__ __launch_bounds__(256) void lc_carry_dc_kernel(float* __restrict__ dcin, const float* __restrict__ dcc, int n) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < n) dcin[e] += dcc[e];
}

void launch_lc_carry_out(const float* part, int np, const float* dcs, const int* wlen_k, float* drow, float* dcc, int Bp, int Hp,
                         int DH, hipStream_t st) {
  hipLaunchKernelGGL(lc_carry_out_kernel, dim3((Bp * Hp + 255) / 256), dim3(256), 0, st, part, np, dcs, wlen_k, drow, dcc, Bp, Hp, DH);
}
void launch_lc_carry_dc(float* dcin, const float* dcc, int n, hipStream_t st) {
  hipLaunchKernelGGL(lc_carry_dc_kernel, dim3((n + 255) / 256), dim3(256), 0, st, dcin, dcc, n);
}

}  // namespace nasr
