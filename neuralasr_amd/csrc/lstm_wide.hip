// lstm_wide.hip — the forward recurrence of a WIDE layer (Hp = 2048, DeepSpeech's cell count: networks/deepspeech.py:70-103)
// as one persistent launch per direction.
//
// Same semantics and buffers as lstm.hip / lstm_persist.hip.  Why a third form: the
// persistent kernels of lstm_persist.hip keep a direction's recurrent matrix in the registers of ONE XCD (Hp <= 512);
// at Hp = 2048 a direction's U is 64 MB — half the chip's register files — and the per-timestep launches of lstm.hip
// re-stream it through the fabric every step (30 us per step, fp32 MFMA floor 13.7 us besides).  Here:
//
//   * ONE direction per launch, its U resident in the registers of all 256 CUs: 256 KB per CU = 8 waves x 128 VGPRs,
//     as two fp16 planes under per-column power-of-two scales (the form of lstm_persist.hip's forward kernel).
//   * the CUs form a 2-D grid.  XCD x owns the CONTRACTION rows of hidden units [KS*x, KS*x + KS) (KS = Hp/8 = 256);
//     member nb of every XCD owns the gate columns of units {KS*x' + 8*nb + i : x' < 8, i < 8}: 8 units from each row
//     slice.  Wave w of a workgroup holds the columns that belong to slice x' = w.
//   * per timestep two hand-offs: (1) h_{s-1} of the XCD's own row slice through the XCD's L2 (32 producers x 1 KB,
//     plain stores + sc1 loads, as lstm_persist.hip); (2) the 8 partial sums of every unit cross the XCDs: wave w
//     sends its 16*MT x 32 partial pre-activations to workgroup (w, nb) (sc1 write-through stores, no flag), which sums
//     the 8 in fixed order, does the cell update of its 8 units (c in a register for all T) and publishes h.
//   * products on v_mfma_f32_16x16x32_f16: 2h split into two fp16 parts by its producer, three products per tile.  The
//     parts carry the epoch of their buffer's use, so the loads of hand-off (1) validate themselves.
//
// Placement is read from HW_REG_XCC_ID with a ticket per XCD; every spin is bounded; a timeout or an unexpected placement
// raises WideCtl::error (+ the sticky host word and the fault float) and the launch drains.
#include "kernels.h"
#include "lstm_device.h"

#include <cstdlib>

#ifndef NASR_WSTAMP
#define NASR_WSTAMP 0   // 1: s_memtime deltas per phase -> WideCtl::stamps (tools/widebench)
#endif

namespace nasr {

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int PF = 2;   // k-tiles of A fragments read ahead of the MFMAs (widebench A/B: 1, 2, 3)

__device__ __forceinline__ u32x4 ld16_sc1(const void* p) {
  u32x4 v;
  asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(v) : "v"(p) : "memory");
  return v;
}
// (the compiler's hazard recogniser does not look inside inline asm: a VALU write of the data registers in the slot right
//  behind a store of more than 8 bytes corrupts the tail of the store, hence the s_nop)
__device__ __forceinline__ void st16_sc1(void* p, f32x4 v) {
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(v) : "memory");
}
// wait for the asm loads above; the loaded value passes through the statement so that no copy of it is scheduled earlier
__device__ __forceinline__ void wait_vm0(u32x4& v) { asm volatile("s_waitcnt vmcnt(0)" : "+v"(v) : : "memory"); }

// Sentinel-polled inboxes: a block with ONE reader holds the sentinel (all ones, a NaN no arithmetic produces) until the data
// land, so its words are polled themselves - no flag - and reset by the reader for the step after next.
constexpr unsigned SENTINEL = 0xffffffffu;
// every word of this 16-byte granule differs from the sentinel
__device__ __forceinline__ bool landed(u32x4 t) { return t.x != SENTINEL && t.y != SENTINEL && t.z != SENTINEL && t.w != SENTINEL; }
// loads the [MT][2] granules per lane at src (64 apart) until every word of every lane has landed; the granule stored last
// first: when it is there the others mostly are.  false: the spin budget ran out.
template <int MT>
__device__ __forceinline__ bool poll_landed(const u32x4* src, u32x4 (&v)[MT][2]) {
  for (unsigned n = 0; n < SPIN_BUDGET; ++n) {
    v[MT - 1][1] = ld16_sc1(src + ((MT - 1) * 2 + 1) * 64);
    wait_vm0(v[MT - 1][1]);
    if (!__all(landed(v[MT - 1][1]))) continue;
    bool all = true;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int p = 0; p < 2; ++p)
        if (m != MT - 1 || p != 1) v[m][p] = ld16_sc1(src + (m * 2 + p) * 64);
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int p = 0; p < 2; ++p)
        if (m != MT - 1 || p != 1) {
          wait_vm0(v[m][p]);
          all = all && landed(v[m][p]);
        }
    if (__all(all)) return true;
  }
  return false;
}

// every wave of workgroups (0,0) and (7,31) stamps its phases -> WideCtl::stamps [16 waves][10]
using WStamps = Stamps<10, NASR_WSTAMP != 0>;

}  // namespace

// ------------------------------------------------------------------ operand image
// U canonical [Hp][N4] (row k = h unit, column 4*j + g), cs [N4] power-of-two column scales.
// Uw as 16-byte units [8 x][32 nb][8 w][8 kt][2 h2][2 plane][64 lane]: lane l holds the 8 halfs
//   U[k = KS*x + 32*kt + 8*(l>>4) + 0..7][col = 4*(KS*w + 8*nb + 4*h2 + ((l&15)>>2)) + (l&3)] * cs[col],
//   plane 0 = fp16(v), plane 1 = fp16(v - plane 0): the B operand of v_mfma_f32_16x16x32_f16.
__global__ __launch_bounds__(256) void repack_wide_kernel(const float* __restrict__ U, const float* __restrict__ cs,
                                                          u32x4* __restrict__ Uw, int Hp) {
  const int KS = Hp / 8, N4 = 4 * Hp;
  const int64_t total = (int64_t)8 * 32 * 8 * 8 * 2 * 64;   // (x, nb, w, kt, h2, lane)
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int l = (int)(e & 63);
    int64_t r = e >> 6;
    const int h2 = (int)(r & 1); r >>= 1;
    const int kt = (int)(r & 7); r >>= 3;
    const int w = (int)(r & 7); r >>= 3;
    const int nb = (int)(r & 31), x = (int)(r >> 5);
    const int col = 4 * (KS * w + 8 * nb + 4 * h2 + ((l & 15) >> 2)) + (l & 3);
    const int k0 = KS * x + 32 * kt + 8 * (l >> 4);
    const float sc = cs[col];
    h8 p1, p2;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = U[(size_t)(k0 + j) * N4 + col] * sc;
      _Float16 a, b;
      split_f16x2(v, a, b);
      p1[j] = a;
      p2[j] = b;
    }
    u32x4* dst = Uw + (e >> 6) * 128 + l;
    dst[0] = __builtin_bit_cast(u32x4, p1);
    dst[64] = __builtin_bit_cast(u32x4, p2);
  }
}

size_t wide_image_bytes(int Hp) { return (size_t)Hp * 4 * Hp * 4; }
bool wide_supported(int Hp, int Bp) { return Hp == 2048 && Bp >= 16 && Bp <= 64 && Bp % 16 == 0; }
size_t wide_hx_bytes(int Bp) { return (size_t)2 * 8 * 32 * 2 * Bp * 16; }
size_t wide_part_bytes(int Bp) { return (size_t)2 * 256 * 8 * (Bp / 16) * 2 * 64 * 16; }

void launch_repack_wide(const float* U, const float* cs, void* Uw, int Hp, hipStream_t st) {
  hipLaunchKernelGGL(repack_wide_kernel, dim3(2048), dim3(256), 0, st, U, cs, reinterpret_cast<u32x4*>(Uw), Hp);
}

// ------------------------------------------------------------------ forward
// LDS map (16-byte units): A [8 kt][MT][2 p][64] | P [8 src][MT][2 h2][64] | hp [2 p][16*MT rows] | info
template <int MT>
struct WideLds {
  static constexpr int A = 0, P = A + 8 * MT * 2 * 64, HP = P + 8 * MT * 2 * 64, INFO = HP + 2 * 16 * MT, END = INFO + 4;
};

template <int MT>
__global__ __launch_bounds__(512, 1) void lstm_wide_fwd_kernel(
    const u32x4* __restrict__ Uw,       // this direction's image
    float* gates, float* cbuf, float* out, const int* __restrict__ seq_len,
    u32x4* hx,                           // [2 parity][8 x][32 nb][2 plane][16*MT rows]: 8 halfs of 2h per unit
    float* part,                         // [2 parity][256 dest][8 src][MT][2 h2][64 lane][4]
    WideCtl* ctl, unsigned* sticky, WideGeom gm, float fb, const float* __restrict__ cinv) {
  extern __shared__ __attribute__((aligned(16))) u32x4 wlds[];
  using L = WideLds<MT>;
  constexpr int ROWS = 16 * MT;
  constexpr int NCW = (8 * ROWS + 63) / 64;      // waves with cell threads
  u32x4* Alds = wlds + L::A;
  f32x4* Plds = reinterpret_cast<f32x4*>(wlds + L::P);
  _Float16* hp = reinterpret_cast<_Float16*>(wlds + L::HP);
  unsigned* info = reinterpret_cast<unsigned*>(wlds + L::INFO);
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;

  // ---- placement: XCD id = row slice x, ticket = member nb
  unsigned xcc, member;
  if (!join_xcd(ctl, sticky, gm.fault, info, 2, xcc, member)) return;
  const int x = (int)xcc, nb = (int)member;
  const int T = gm.T, Bp = gm.Bp, Hp = gm.Hp, D = gm.D, d = gm.d;
  const int KS = Hp / 8, N4 = 4 * Hp, DH = D * Hp, DN = D * N4;
  const int me = x * 32 + nb;

  // ---- this wave's 256 x 32 block of U (destination slice w), resident for the whole launch: 128 VGPRs
  h8 ur[8][2][2];
  {
    const u32x4* up = Uw + ((size_t)(me * 8 + w) * 8) * 4 * 64 + lane;
#pragma unroll
    for (int kt = 0; kt < 8; ++kt)
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
        for (int p = 0; p < 2; ++p) ur[kt][h2][p] = __builtin_bit_cast(h8, up[((kt * 2 + h2) * 2 + p) * 64]);
  }
  float osc[2];
#pragma unroll
  for (int h2 = 0; h2 < 2; ++h2)
    osc[h2] = cinv[4 * (KS * w + 8 * nb + 4 * h2 + ((lane & 15) >> 2)) + (lane & 3)] * 0.5f;   // h travels as 2h

  // ---- cell threads: tid < 128*MT: (row b, unit i of this workgroup's 8)
  const bool cell = tid < 8 * ROWS;
  const int cb = tid >> 3, ci = tid & 7;
  const int u = KS * x + 8 * nb + ci;
  const int len = (cell && cb < Bp) ? seq_len[cb] : 0;
  const bool rowok = cell && cb < Bp;
  float c = 0.f;
  const unsigned xstep = (unsigned)Bp * (unsigned)DN;
  const unsigned xoff = (unsigned)(rowok ? cb : 0) * (unsigned)DN + (unsigned)(d * N4 + 4 * u);
  auto frame_of = [&](int s) { return (rowok && s < len) ? (d ? len - 1 - s : s) : 0; };
  bool aborted = false;
  WStamps stp;
  stp.start(me == 0 || me == 255);

  for (int s = 0; s < T; ++s) {
    const int par = s & 1;
    bool ok = true;
    stp.mark(0);
    // gate pre-activations of this step's frame (x W + b, from the hoisted GEMM): in flight during the whole product phase
    f32x4 xg = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (cell) xg = *reinterpret_cast<const f32x4*>(gates + (xoff + (unsigned)frame_of(s) * xstep));

    if (s > 0) {
      // 1. h_{s-1} of this XCD's row slice: wave w fetches k-tile w = the 8 units of producers 4w .. 4w+3
      const u32x4* src = hx + ((size_t)(((s - 1) & 1) * 8 + x) * 32 + 4 * w + (lane >> 4)) * 2 * ROWS + (lane & 15);
      u32x4 v[MT][2];
      // ONE round trip, as in lstm_persist.hip: every half of the two planes carries the epoch of this use of the buffer in
      // bit 14 (plane 0 = fp16(2h), plane 1 = fp16((2h - plane 0) * 2^10): both stay below 2, their exponent fields below
      // 16), so the loads themselves say whether the four producers have published; a lane with a stale granule loads
      // again.  Waves without cell threads first wait (in LDS) until this workgroup's own cell waves have published.
      ok = !(s == gm.inject && me == 0);
      if (ok) {
        const unsigned want = (unsigned)s * (unsigned)NCW;
        for (unsigned n = 0; n < (1u << 24) && (int)(*(lds_vu32*)(info + 3) - want) < 0; ++n)
          __builtin_amdgcn_s_sleep(1);
      }
      stp.mark(1);
      if (ok) {
        const unsigned em = use_epoch(0, T, s - 1) ? 0x40004000u : 0u;
        bool need = true;
        ok = false;
        for (unsigned n = 0; n < SPIN_BUDGET; ++n) {
          if (need) {
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
              for (int p = 0; p < 2; ++p) v[m][p] = ld16_sc1(src + p * ROWS + 16 * m);
          }
          unsigned bad = 0;
#pragma unroll
          for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int p = 0; p < 2; ++p) {
              wait_vm0(v[m][p]);
              const u32x4 t = v[m][p];
              bad |= (t.x ^ em) | (t.y ^ em) | (t.z ^ em) | (t.w ^ em);
            }
          need = (bad & 0x40004000u) != 0;
          if (!__any(need)) { ok = true; break; }
        }
      }
      if (ok) {
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int p = 0; p < 2; ++p) {
            u32x4 t = v[m][p];
            t.x &= 0xBFFFBFFFu; t.y &= 0xBFFFBFFFu; t.z &= 0xBFFFBFFFu; t.w &= 0xBFFFBFFFu;
            Alds[((w * MT + m) * 2 + p) * 64 + lane] = t;
          }
      } else {
        info[2] = 1;
      }
    }
    stp.mark(2);
    __syncthreads();                                        // #1: the A operand is in LDS
    stp.mark(3);
    if (s > 0 && !info[2]) {
      // 2. + 3. partial pre-activations of destination slice w over this XCD's 256 contraction rows, one 16 x 16 tile
      // at a time; each tile leaves for workgroup (w, nb) as soon as it is complete (its write-through acknowledgement
      // overlaps the MFMAs of the next tile); the own slice stays in LDS
      float* pdst = part + ((((size_t)par * 256 + (w * 32 + nb)) * 8 + x) * MT * 2) * 256 + lane * 4;
      // (the sentinel stores this wave made as a CONSUMER one step ago are acknowledged: whoever sees the partial sums
      //  below and later overwrites a slot this wave reset finds the reset already in memory)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      stp.mark(5);
      static_for<0, MT>([&](auto mc) {
        constexpr int m = decltype(mc)::value;
        // both 16 x 16 tiles of this M tile together; the A fragments of k-tile kt+1 are read while kt multiplies (the
        // scheduling barriers keep the compiler from hoisting every read to the top, which costs 64 registers per M tile)
        f32x4 t0 = (f32x4){0.f, 0.f, 0.f, 0.f}, t1 = (f32x4){0.f, 0.f, 0.f, 0.f};
        f32x4 t0b = (f32x4){0.f, 0.f, 0.f, 0.f}, t1b = (f32x4){0.f, 0.f, 0.f, 0.f};   // the plane-1 products (scale 2^11 instead of 2)
        // fragments of k-tiles kt+1 and kt+2 are in flight while kt multiplies (PF = prefetch distance)
        h8 q0[PF + 1], q1[PF + 1];
#pragma unroll
        for (int j = 0; j < PF; ++j) {
          q0[j] = __builtin_bit_cast(h8, Alds[((j * MT + m) * 2 + 0) * 64 + lane]);
          q1[j] = __builtin_bit_cast(h8, Alds[((j * MT + m) * 2 + 1) * 64 + lane]);
        }
        static_for<0, 8>([&](auto ktc) {
          constexpr int kt = decltype(ktc)::value;
          if constexpr (kt + PF < 8) {
            q0[(kt + PF) % (PF + 1)] = __builtin_bit_cast(h8, Alds[(((kt + PF) * MT + m) * 2 + 0) * 64 + lane]);
            q1[(kt + PF) % (PF + 1)] = __builtin_bit_cast(h8, Alds[(((kt + PF) * MT + m) * 2 + 1) * 64 + lane]);
          }
          const h8 c0 = q0[kt % (PF + 1)], c1 = q1[kt % (PF + 1)];
          t0b = __builtin_amdgcn_mfma_f32_16x16x32_f16(c1, ur[kt][0][0], t0b, 0, 0, 0);
          t1b = __builtin_amdgcn_mfma_f32_16x16x32_f16(c1, ur[kt][1][0], t1b, 0, 0, 0);
          t0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(c0, ur[kt][0][1], t0, 0, 0, 0);
          t1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(c0, ur[kt][1][1], t1, 0, 0, 0);
          t0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(c0, ur[kt][0][0], t0, 0, 0, 0);
          t1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(c0, ur[kt][1][0], t1, 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        });
        t0 = t0 + t0b * (1.f / 1024.f);
        t1 = t1 + t1b * (1.f / 1024.f);
        t0 *= osc[0];
        t1 *= osc[1];
        if (w != x) {
          st16_sc1(pdst + (m * 2 + 0) * 256, t0);
          st16_sc1(pdst + (m * 2 + 1) * 256, t1);
        } else {
          Plds[((x * MT + m) * 2 + 0) * 64 + lane] = t0;
          Plds[((x * MT + m) * 2 + 1) * 64 + lane] = t1;
        }
      });
      stp.mark(4);
      // 4. the 7 partial sums of the own units that other XCDs computed: wave w fetches source slice w from its
      // sentinel-polled inbox, then resets it for the step after next (this parity's next use).
      if (w != x) {
        u32x4* src = reinterpret_cast<u32x4*>(part) + ((((size_t)par * 256 + me) * 8 + w) * MT * 2) * 64 + lane;
        u32x4 v[MT][2];
        ok = poll_landed<MT>(src, v);
        stp.mark(6);
        if (ok) {
          const f32x4 sent = __builtin_bit_cast(f32x4, (u32x4){SENTINEL, SENTINEL, SENTINEL, SENTINEL});
#pragma unroll
          for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {
              Plds[((w * MT + m) * 2 + h2) * 64 + lane] = __builtin_bit_cast(f32x4, v[m][h2]);
              st16_sc1(src + (m * 2 + h2) * 64, sent);
            }
        } else {
          info[2] = 1;
        }
      }
    }
    stp.mark(7);
    __syncthreads();                                        // #2: the 8 partial sums are in LDS
    stp.mark(8);
    const unsigned abort_word = info[2];
    // 5. cell update of (row cb, unit ci): sum of the 8 sources in fixed order
    if (cell) {
      const bool valid = rowok && s < len;
      f32x4 g = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (s > 0) {
        const float* pl = reinterpret_cast<const float*>(Plds) +
                          (((cb >> 4) * 2 + (ci >> 2)) * 64 + 16 * ((cb & 15) >> 2) + 4 * (ci & 3)) * 4 + (cb & 3);
#pragma unroll
        for (int sx = 0; sx < 8; ++sx) {
          const float* ps = pl + sx * MT * 2 * 256;
          g.x += ps[0]; g.y += ps[4]; g.z += ps[8]; g.w += ps[12];
        }
      }
      const f32x4 pre = xg + g;
      const f32x4 act = lstm_gates(pre, fb);
      float h = 0.f;
      if (valid) h = lstm_state(act, c);
      // (|2h| is kept below 2 - tanh and the sigmoid saturate to exactly 1 - so that plane 0's exponent field stays below 16;
      //  the residual of that clamp, 2^-10, is exact in plane 1)
      const float hv = fminf(fmaxf(h * 2.f, -1.9990234375f), 1.9990234375f);
      const _Float16 h1 = (_Float16)hv;
      const _Float16 h2v = (_Float16)((h * 2.f - (float)h1) * 1024.f);
      // bit 14 of every half = the epoch of this use of the buffer
      const unsigned short eb = use_epoch(0, T, s) ? 0x4000u : 0u;
      reinterpret_cast<unsigned short*>(hp)[(0 * ROWS + cb) * 8 + ci] = __builtin_bit_cast(unsigned short, h1) | eb;
      reinterpret_cast<unsigned short*>(hp)[(1 * ROWS + cb) * 8 + ci] = __builtin_bit_cast(unsigned short, h2v) | eb;
      __builtin_amdgcn_wave_barrier();
      // the row's 8 halfs were written by 8 consecutive lanes of this wave: LDS operations of one wave complete in order
      if (ci == 0) {
        u32x4* dst = hx + ((size_t)(par * 8 + x) * 32 + nb) * 2 * ROWS + cb;
        dst[0] = *reinterpret_cast<const u32x4*>(hp + (0 * ROWS + cb) * 8);     // plain stores: land in this XCD's L2
        dst[ROWS] = *reinterpret_cast<const u32x4*>(hp + (1 * ROWS + cb) * 8);
      }
      // no acknowledgement to wait for and no flag: the granules validate themselves.  The workgroup's other waves learn
      // from an LDS counter that this cell wave has published.
      if (lane == 0) atomicAdd(info + 3, 1u);
      // per-frame results for the BPTT / the layer above
      if (rowok) {
        if (valid) {
          const unsigned r = (unsigned)((d ? (len - 1 - s) : s) * Bp + cb);
          *reinterpret_cast<f32x4*>(gates + (r * (unsigned)DN + (unsigned)(d * N4 + 4 * u))) = act;
          const unsigned oc = r * (unsigned)DH + (unsigned)(d * Hp + u);
          cbuf[oc] = c;
          out[oc] = h;
        } else {
          out[(unsigned)(s * Bp + cb) * (unsigned)DH + (unsigned)(d * Hp + u)] = 0.f;   // frame s is past seq_len in both directions
        }
      }
    }
    stp.mark(9);
    if (abort_word) { aborted = true; break; }
  }
  stp.flush(ctl->stamps + ((me ? 8 : 0) + w) * 10);
  if (aborted && tid == 0) raise_error(ctl, sticky, gm.fault, 1u);
}

// ------------------------------------------------------------------ BPTT
// The same 2-D grid with the two hand-offs the other way round.  Per timestep (s descending, k = T-1-s counts them):
//   1. dG of step k-1 - [rows x 32 gate columns] from each of the 8 workgroups (x', nb) that own this workgroup's columns -
//      arrives across the XCDs as two fp16 planes of dG * S_row (power-of-two scale per utterance, wide_row_scale_kernel);
//      sentinel-polled inboxes as in the forward kernel, one copy per reader;
//   2. partial dh of the XCD's 256 units over this workgroup's 256 gate columns: A = dG planes, B = U^T planes under
//      per-unit (row of U) scales, three products; wave w owns units [32w, 32w+32) of the slice = members 4w .. 4w+3;
//   3. XCD-local reduce-scatter through the L2: 32 sources x [rows x 8 units] per workgroup, sentinel-polled like the inboxes
//      (every (destination, source) block has one reader);
//   4. cell backward of the 8 own units (dc in a register for all T), dG to HBM (frame-indexed, for the weight-gradient
//      GEMMs) and, as planes, to the 8 inboxes.
// A dG * S_row beyond the fp16 range raises error bit 2: the launch drains and the step is void (the caller repeats it on
// the per-step kernels).
//
// Uwb as 16-byte units [8 x][32 nb][8 w][8 kt][2 nt][2 plane][64 lane]: lane l holds the 8 halfs
//   U[row = KS*x + 32*w + 16*nt + (l&15)][col = 4*(KS*kt + 8*nb + 2*(l>>4) + (j>>2)) + (j&3)] * rs[row],  j = 0..7.
__global__ __launch_bounds__(256) void repack_wide_bwd_kernel(const float* __restrict__ U, const float* __restrict__ rs,
                                                              u32x4* __restrict__ Uwb, int Hp) {
  const int KS = Hp / 8, N4 = 4 * Hp;
  const int64_t total = (int64_t)8 * 32 * 8 * 8 * 2 * 64;   // (x, nb, w, kt, nt, lane)
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int l = (int)(e & 63);
    int64_t r = e >> 6;
    const int nt = (int)(r & 1); r >>= 1;
    const int kt = (int)(r & 7); r >>= 3;
    const int w = (int)(r & 7); r >>= 3;
    const int nb = (int)(r & 31), x = (int)(r >> 5);
    const int row = KS * x + 32 * w + 16 * nt + (l & 15);
    const float sc = rs[row];
    const float* src = U + (size_t)row * N4 + 4 * (KS * kt + 8 * nb + 2 * (l >> 4));   // 8 consecutive columns: 2 units x 4 gates
    h8 p1, p2;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = src[j] * sc;
      _Float16 a, b;
      split_f16x2(v, a, b);
      p1[j] = a;
      p2[j] = b;
    }
    u32x4* dst = Uwb + (e >> 6) * 128 + l;
    dst[0] = __builtin_bit_cast(u32x4, p1);
    dst[64] = __builtin_bit_cast(u32x4, p2);
  }
}

void launch_repack_wide_bwd(const float* U, const float* rs, void* Uwb, int Hp, hipStream_t st) {
  hipLaunchKernelGGL(repack_wide_bwd_kernel, dim3(2048), dim3(256), 0, st, U, rs, reinterpret_cast<u32x4*>(Uwb), Hp);
}

// smax [D][Bp] (zeroed by the launcher): bits of the largest |dOut| over the frames and units of every (direction, utterance);
// non-negative floats order like their bit patterns, so the partial maxima of the (utterance, direction, time chunk) blocks
// meet in an atomicMax.  The BPTT kernel turns it into the power-of-two scale S that brings that maximum into [2^5, 2^6)
// (1 where the utterance has no gradient): dG = O(dOut) then has 2^10 of headroom in the fp16 planes.
constexpr int WIDE_SCALE_CHUNK = 16;   // frames per block
__global__ __launch_bounds__(256) void wide_row_max_kernel(const float* __restrict__ dout, const int* __restrict__ seq_len,
                                                           unsigned* __restrict__ smax, int T, int Bp, int Hp, int D) {
  __shared__ float red[256];
  const int b = blockIdx.x, d = blockIdx.y, DH = D * Hp;
  const int len = seq_len[b] < T ? seq_len[b] : T;
  const int t0 = blockIdx.z * WIDE_SCALE_CHUNK, t1 = t0 + WIDE_SCALE_CHUNK < len ? t0 + WIDE_SCALE_CHUNK : len;
  if (t0 >= len) return;
  float m = 0.f;
  for (int t = t0; t < t1; ++t) {
    const float4* row = reinterpret_cast<const float4*>(dout + ((size_t)t * Bp + b) * DH + d * Hp);
    for (int j = threadIdx.x; j < Hp / 4; j += 256) {
      const float4 v = row[j];
      m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
  }
  red[threadIdx.x] = m;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0 && red[0] > 0.f) atomicMax(&smax[d * Bp + b], __float_as_uint(red[0]));
}

__device__ __forceinline__ float wide_scale_of(unsigned maxbits, int shift) {
  const float mx = __uint_as_float(maxbits);
  if (!(mx > 0.f && mx < 3e38f)) return 1.f;
  int e;
  (void)frexpf(mx, &e);                 // mx = f * 2^e, f in [0.5, 1)
  return ldexpf(1.f, 6 - e + shift);    // mx * S in [2^5, 2^6) (shift: test hook NASR_WIDE_SCALE_SHIFT)
}

// LDS map (16-byte units): A [8 kt][MT][2 p][64] | PB [32 src][32*MT] | sinv [16*MT floats] | info
template <int MT>
struct WideLdsB {
  static constexpr int A = 0, PB = A + 8 * MT * 2 * 64, SINV = PB + 32 * 32 * MT, INFO = SINV + 4 * MT, END = INFO + 4;
};

template <int MT>
__global__ __launch_bounds__(512, 1) void lstm_wide_bwd_kernel(
    const u32x4* __restrict__ Uwb,      // this direction's backward image
    const float* __restrict__ gates,    // activations si,tj,sf,so [R][D*N4]
    float* dgbuf,                       // dG, frame-indexed [R][D*N4]
    const float* __restrict__ cbuf, const float* __restrict__ dout, const int* __restrict__ seq_len,
    u32x4* inbox,                       // [2 parity][256 dest][8 src][MT][2 plane][64 lane]: dG planes in A-fragment order
    f32x4* px,                          // [2 parity][8 x][32 dest][32 src][32*MT]: partial dh, [m][unit 8][q 4] x 4 rows
    WideCtl* ctl, unsigned* sticky, WideGeom gm, const float* __restrict__ rinv,   // [Hp] 1 / row scale of U
    const unsigned* __restrict__ smax) {   // [Bp] bits of max |dOut| per utterance of this direction (wide_row_max_kernel)
  extern __shared__ __attribute__((aligned(16))) u32x4 wlds[];
  using L = WideLdsB<MT>;
  constexpr int ROWS = 16 * MT, PU = 32 * MT;     // PU: 16-byte units of one [rows x 8 units] partial block
  u32x4* Alds = wlds + L::A;
  f32x4* PBlds = reinterpret_cast<f32x4*>(wlds + L::PB);
  unsigned* info = reinterpret_cast<unsigned*>(wlds + L::INFO);
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  unsigned xcc, member;
  if (!join_xcd(ctl, sticky, gm.fault, info, 2, xcc, member)) return;
  const int x = (int)xcc, nb = (int)member;
  const int T = gm.T, Bp = gm.Bp, Hp = gm.Hp, D = gm.D, d = gm.d;
  const int KS = Hp / 8, N4 = 4 * Hp, DH = D * Hp, DN = D * N4;
  const int me = x * 32 + nb;

  // ---- this wave's block of U^T: units [32w, 32w+32) of the slice x over the workgroup's 256 gate columns
  h8 ub[8][2][2];
  {
    const u32x4* up = Uwb + ((size_t)(me * 8 + w) * 8) * 4 * 64 + lane;
#pragma unroll
    for (int kt = 0; kt < 8; ++kt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int p = 0; p < 2; ++p) ub[kt][nt][p] = __builtin_bit_cast(h8, up[((kt * 2 + nt) * 2 + p) * 64]);
  }
  // output scale of C element (row 16m + 4(l>>4) + r, unit 32w + 16nt + (l&15)): 1 / (row scale of U x S of the utterance)
  float oun[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) oun[nt] = rinv[KS * x + 32 * w + 16 * nt + (lane & 15)];
  float* sinv = reinterpret_cast<float*>(wlds + L::SINV);     // 1 / S of every utterance row (read back per tile)
  if (tid < ROWS) sinv[tid] = tid < Bp ? 1.f / wide_scale_of(smax[tid], gm.scale_shift) : 1.f;
  __syncthreads();

  // ---- cell threads
  const bool cell = tid < 8 * ROWS;
  const int cb = tid >> 3, ci = tid & 7;
  const int u = KS * x + 8 * nb + ci;
  const bool rowok = cell && cb < Bp;
  const int len = rowok ? seq_len[cb] : 0;
  const float sb = rowok ? wide_scale_of(smax[cb], gm.scale_shift) : 1.f;
  float dc = 0.f;
  bool aborted = false;
  WStamps stp;
  stp.start(me == 0 || me == 255);
  const f32x4 sent = __builtin_bit_cast(f32x4, (u32x4){SENTINEL, SENTINEL, SENTINEL, SENTINEL});

  for (int k = 0; k < T; ++k) {
    const int s = T - 1 - k, par = k & 1;
    bool ok = true;
    stp.mark(0);
    // per-frame operands of the cell backward: in flight during the gather / product phases.  Unconditional loads
    // (a masked cell reads frame 0 of its row and is zeroed below).
    const bool valid = rowok && s < len;
    const int tb = valid ? (d ? len - 1 - s : s) : 0;
    const unsigned r_ = (unsigned)(tb * Bp + (rowok ? cb : 0));
    const unsigned rp = s > 0 ? (d ? r_ + Bp : r_ - Bp) : r_;
    f32x4 act = (f32x4){0.f, 0.f, 0.f, 0.f};
    float cc = 0.f, cpv = 0.f, dh = 0.f;
    auto load_cell = [&]() {
      if (cell) {
        act = *reinterpret_cast<const f32x4*>(gates + (r_ * (unsigned)DN + (unsigned)(d * N4 + 4 * u)));
        cc = cbuf[r_ * (unsigned)DH + (unsigned)(d * Hp + u)];
        cpv = cbuf[(valid ? rp : r_) * (unsigned)DH + (unsigned)(d * Hp + u)];
        dh = dout[r_ * (unsigned)DH + (unsigned)(d * Hp + u)];
      }
    };
    if (k == 0) load_cell();
    if (k > 0) {
      // 1. dG of step k-1 from source slice w (its 32 gate columns of this workgroup's 256): the own slice is already in LDS
      if (w != x) {
        u32x4* src = inbox + ((((size_t)((k - 1) & 1) * 256 + me) * 8 + w) * MT * 2) * 64 + lane;
        u32x4 v[MT][2];
        ok = poll_landed<MT>(src, v);
        if (s == gm.inject && me == 0) ok = false;
        stp.mark(1);
        if (ok) {
#pragma unroll
          for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int p = 0; p < 2; ++p) {
              Alds[((w * MT + m) * 2 + p) * 64 + lane] = v[m][p];
              st16_sc1(src + (m * 2 + p) * 64, sent);
            }
        } else {
          info[2] = 1;
        }
      }
    }
    stp.mark(2);
    __syncthreads();                                        // #1: dG of step k-1 is in LDS (all 8 column groups)
    stp.mark(3);
    if (k > 0 && !info[2]) {
      // 2. partial dh of units [32w, 32w+32) of the slice; each 16 x 16 tile goes to the XCD's exchange buffer at once
      f32x4* pdst = px + (((size_t)(par * 8 + x) * 32) * 32 + nb) * PU;        // + dest * 32 * PU
      // (the sentinels this wave wrote as a READER one step ago are acknowledged before it writes as a source again: whoever
      //  sees the partial sums below and later refills a block this wave reset finds the reset in the L2 already)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      static_for<0, MT>([&](auto mc) {
        constexpr int m = decltype(mc)::value;
        // both 16 x 16 tiles of this M tile together; the A fragments of k-tile kt+1 are read while kt multiplies (the
        // scheduling barriers keep the compiler from hoisting every read to the top, which costs 64 registers per M tile)
        f32x4 t0 = (f32x4){0.f, 0.f, 0.f, 0.f}, t1 = (f32x4){0.f, 0.f, 0.f, 0.f};
        // fragments of k-tiles kt+1 and kt+2 are in flight while kt multiplies (PF = prefetch distance)
        h8 q0[PF + 1], q1[PF + 1];
#pragma unroll
        for (int j = 0; j < PF; ++j) {
          q0[j] = __builtin_bit_cast(h8, Alds[((j * MT + m) * 2 + 0) * 64 + lane]);
          q1[j] = __builtin_bit_cast(h8, Alds[((j * MT + m) * 2 + 1) * 64 + lane]);
        }
        static_for<0, 8>([&](auto ktc) {
          constexpr int kt = decltype(ktc)::value;
          if constexpr (kt + PF < 8) {
            q0[(kt + PF) % (PF + 1)] = __builtin_bit_cast(h8, Alds[(((kt + PF) * MT + m) * 2 + 0) * 64 + lane]);
            q1[(kt + PF) % (PF + 1)] = __builtin_bit_cast(h8, Alds[(((kt + PF) * MT + m) * 2 + 1) * 64 + lane]);
          }
          const h8 c0 = q0[kt % (PF + 1)], c1 = q1[kt % (PF + 1)];
          t0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(c1, ub[kt][0][0], t0, 0, 0, 0);
          t1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(c1, ub[kt][1][0], t1, 0, 0, 0);
          t0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(c0, ub[kt][0][1], t0, 0, 0, 0);
          t1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(c0, ub[kt][1][1], t1, 0, 0, 0);
          t0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(c0, ub[kt][0][0], t0, 0, 0, 0);
          t1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(c0, ub[kt][1][0], t1, 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        });
        const f32x4 si = *reinterpret_cast<const f32x4*>(sinv + 16 * m + 4 * (lane >> 4));
        t0 *= si * oun[0];
        t1 *= si * oun[1];
        // unit 32w + 16nt + (l&15) belongs to member 4w + 2nt + ((l&15)>>3), its unit (l&7); rows 16m + 4(l>>4) + 0..3
        const int dest = 4 * w + ((lane & 15) >> 3);
        f32x4* pd = pdst + (size_t)dest * 32 * PU + ((m * 8 + (lane & 7)) * 4 + (lane >> 4));   // plain stores: this XCD's L2
        pd[0] = t0;
        pd[(size_t)2 * 32 * PU] = t1;
      });
      stp.mark(4);
      load_cell();                                           // in flight under the gather below
      stp.mark(5);
      // 3. the 32 partial sums of the own 8 units: wave w fetches sources 4w .. 4w+3.  No flag, as across the XCDs: every
      // (destination, source) block has ONE reader, so its words are polled against the sentinel and reset after the read
      {
        f32x4* src = px + (((size_t)(par * 8 + x) * 32 + nb) * 32 + 4 * w) * PU;
        constexpr int NL = (4 * PU + 63) / 64;               // 16-byte loads per lane for 4 sources
        u32x4 v[NL];
        ok = false;
        for (unsigned n = 0; n < SPIN_BUDGET; ++n) {
          bool all = true;
#pragma unroll
          for (int j = 0; j < NL; ++j)
            if (lane + 64 * j < 4 * PU) v[j] = ld16_sc1(src + lane + 64 * j);
#pragma unroll
          for (int j = 0; j < NL; ++j)
            if (lane + 64 * j < 4 * PU) {
              wait_vm0(v[j]);
              all = all && landed(v[j]);
            }
          if (__all(all)) { ok = true; break; }
        }
        stp.mark(6);
        if (ok) {
#pragma unroll
          for (int j = 0; j < NL; ++j)
            if (lane + 64 * j < 4 * PU) {
              PBlds[4 * w * PU + lane + 64 * j] = __builtin_bit_cast(f32x4, v[j]);
              src[lane + 64 * j] = sent;                     // plain store: this XCD's L2
            }
        } else {
          info[2] = 1;
        }
      }
    }
    stp.mark(7);
    __syncthreads();                                        // #2: the 32 partial sums are in LDS
    stp.mark(8);
    const unsigned abort_word = info[2];
    // 4. cell backward of (row cb, unit ci)
    if (cell) {
      float dhs = dh;
      if (k > 0) {
        const float* pl = reinterpret_cast<const float*>(PBlds) + (((cb >> 4) * 8 + ci) * 4 + ((cb & 15) >> 2)) * 4 + (cb & 3);
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int sx = 0; sx < 32; sx += 2) { s0 += pl[sx * PU * 4]; s1 += pl[(sx + 1) * PU * 4]; }
        dhs += s0 + s1;
      }
      f32x4 dg = (f32x4){0.f, 0.f, 0.f, 0.f};
      float dcn = 0.f;
      if (valid) dg = lstm_cell_bwd(act, cc, cpv, s == 0, dhs, dc, dcn);
      dc = dcn;
      // the planes of dG * S_row in A-fragment order: (row cb, columns 4ci .. 4ci+3) of the 32 = unit (cb&15) + 16*(ci>>1) of
      // M tile cb>>4, halfs 4*(ci&1) ..
      const f32x4 sv = dg * sb;
      if (!(fabsf(sv.x) < 32768.f && fabsf(sv.y) < 32768.f && fabsf(sv.z) < 32768.f && fabsf(sv.w) < 32768.f)) info[3] = 1;
      typedef _Float16 h4 __attribute__((ext_vector_type(4)));
      h4 p1, p2;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        _Float16 a, b;
        split_f16x2(sv[j], a, b);
        p1[j] = a;
        p2[j] = b;
      }
      // own column group (kt = x) of the next step's A operand: straight into LDS
      h4* ap = reinterpret_cast<h4*>(Alds + ((x * MT + (cb >> 4)) * 2) * 64 + (cb & 15) + 16 * (ci >> 1)) + (ci & 1);
      ap[0] = p1;
      ap[64 * 2] = p2;                                       // plane 1: 64 units of 16 bytes = 128 h4 further
      // dG for the weight-gradient GEMMs (zero at masked steps: the frame of a masked step is frame s itself)
      if (rowok) {
        const unsigned row = valid ? r_ : (unsigned)(s * Bp + cb);
        *reinterpret_cast<f32x4*>(dgbuf + (row * (unsigned)DN + (unsigned)(d * N4 + 4 * u))) = dg;
      }
    }
    __syncthreads();                                        // #3: the own dG tile is complete in LDS
    if (info[3]) { if (tid == 0) raise_error(ctl, sticky, gm.fault, 4u); aborted = true; }
    // 5. publish the tile to the 7 other workgroups that hold these units' columns (wave w -> XCD w)
    if (w != x && k + 1 < T && !aborted) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // (the sentinel stores of this wave's gather are acknowledged)
      u32x4* dst = inbox + ((((size_t)par * 256 + (w * 32 + nb)) * 8 + x) * MT * 2) * 64 + lane;
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int p = 0; p < 2; ++p)
          st16_sc1(dst + (m * 2 + p) * 64, __builtin_bit_cast(f32x4, Alds[((x * MT + m) * 2 + p) * 64 + lane]));
    }
    stp.mark(9);
    if (abort_word || aborted) { aborted = true; break; }
  }
  stp.flush(ctl->stamps + ((me ? 8 : 0) + w) * 10);
  if (aborted && tid == 0) raise_error(ctl, sticky, gm.fault, 1u);
}

using WideMT = std::integer_sequence<int, 1, 2, 3, 4>;   // MT = Bp/16 the kernels are built for

hipError_t wide_prepare() {
  hipError_t e = hipSuccess;
  auto raise = [&](auto* kernel, int bytes) {
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  };
  for_each_int(WideMT{}, [&](auto mt) { raise(&lstm_wide_fwd_kernel<mt()>, WideLds<mt()>::END * 16); });
  for_each_int(WideMT{}, [&](auto mt) { raise(&lstm_wide_bwd_kernel<mt()>, WideLdsB<mt()>::END * 16); });
  return e;
}

size_t wide_px_bytes(int Bp) { return (size_t)2 * 8 * 32 * 32 * (32 * (Bp / 16)) * 16; }

void launch_wide_row_scales(const LstmDims& dm, const float* dout, const int* seq_len, float* srow, hipStream_t st) {
  (void)hipMemsetAsync(srow, 0, (size_t)dm.D * dm.Bp * 4, st);
  hipLaunchKernelGGL(wide_row_max_kernel, dim3(dm.Bp, dm.D, (dm.T + WIDE_SCALE_CHUNK - 1) / WIDE_SCALE_CHUNK), dim3(256), 0, st, dout,
                     seq_len, reinterpret_cast<unsigned*>(srow), dm.T, dm.Bp, dm.Hp, dm.D);
}

void launch_lstm_wide_bwd(const LstmDims& dm, int d, const void* Uwb, const float* rinv, const float* srow,
                          const float* gates, float* dgbuf, const float* cbuf, const float* dout, const int* seq_len,
                          float* inbox, void* px, WideCtl* ctl, unsigned* sticky, float* fault, hipStream_t st) {
  (void)hipMemsetAsync(ctl, 0, sizeof(WideCtl), st);
  (void)hipMemsetAsync(inbox, 0xff, wide_part_bytes(dm.Bp), st);   // every inbox word = the sentinel
  (void)hipMemsetAsync(px, 0xff, wide_px_bytes(dm.Bp), st);
  WideGeom gm{dm.T, dm.Bp, dm.Hp, dm.D, d, -1, 0, fault};
  if (const char* e = test_hook("NASR_WIDE_FAULT_BWD")) gm.inject = atoi(e);
  if (const char* e = test_hook("NASR_WIDE_SCALE_SHIFT")) gm.scale_shift = atoi(e);   // test hook: > 10 drives dG * S out of the fp16 range
  dispatch_int(WideMT{}, dm.Bp / 16, [&](auto mt) {
    hipLaunchKernelGGL((lstm_wide_bwd_kernel<mt()>), dim3(256), dim3(512), WideLdsB<mt()>::END * 16, st,
                       reinterpret_cast<const u32x4*>(Uwb), gates, dgbuf, cbuf, dout, seq_len, reinterpret_cast<u32x4*>(inbox),
                       reinterpret_cast<f32x4*>(px), ctl, sticky, gm, rinv, reinterpret_cast<const unsigned*>(srow) + (size_t)d * dm.Bp);
  });
}

void launch_lstm_wide_fwd(const LstmDims& dm, int d, const void* Uw, const float* cinv, float* gates, float* cbuf,
                          float* out, const int* seq_len, void* hx, float* part, WideCtl* ctl, unsigned* sticky,
                          float* fault, float forget_bias, hipStream_t st) {
  (void)hipMemsetAsync(ctl, 0, sizeof(WideCtl), st);
  (void)hipMemsetAsync(part, 0xff, wide_part_bytes(dm.Bp), st);   // every inbox word = the sentinel
  (void)hipMemsetAsync(hx, 0, wide_hx_bytes(dm.Bp), st);   // the h buffers start from epoch 0
  WideGeom gm{dm.T, dm.Bp, dm.Hp, dm.D, d, -1, 0, fault};
  if (const char* e = test_hook("NASR_WIDE_FAULT")) gm.inject = atoi(e);
  dispatch_int(WideMT{}, dm.Bp / 16, [&](auto mt) {
    hipLaunchKernelGGL((lstm_wide_fwd_kernel<mt()>), dim3(256), dim3(512), WideLds<mt()>::END * 16, st,
                       reinterpret_cast<const u32x4*>(Uw), gates, cbuf, out, seq_len, reinterpret_cast<u32x4*>(hx), part, ctl, sticky,
                       gm, forget_bias, cinv);
  });
}

}  // namespace nasr
