// MFMA implicit-GEMM convolution / GEMM for MI355X (gfx950), bf16 NHWC.
//
// One kernel covers the R50 backbone's forward conv shapes:
//   out[n,p,q,co] = sum_{r,s,ci} x[n, p*stride-pad+r, q*stride-pad+s, ci]
//                               * w[co, r, s, ci]            (+bias, +ReLU)
// as the GEMM  C[M,N] = A[M,K] @ Bt[N,K]^T with
//   M = N*P*Q output positions, N = Cout, K = KH*KW*Cin,
//   A rows gathered from the NHWC input on the fly (im2col-free),
//   Bt = the channels_last conv weight as stored ([co][r][s][ci]) — no
//   weight reshape needed.  KH=KW=1, stride=1, pad=0 degenerates to a plain
//   GEMM (fc layers, 1x1 convs).
//
// Structure (cdna_hip_programming.md §5 canonical anatomy, reg-staged):
//   128x128 block tile, BK=64, 4 waves each computing a 64x64 sub-tile as
//   4x4 fragments of v_mfma_f32_16x16x32_bf16; A/B tiles staged via
//   registers into LDS with +16B row padding (bank-conflict fix, §6 G4);
//   fp32 accumulate; fused bias + ReLU epilogue, bf16 store.  The folded-
//   inference entry (conv_fused_fwd_kernel) runs the same tile body with a
//   bias + residual + ReLU epilogue staged through LDS (16-byte stores).
//
// A-fragment layout for mfma_f32_16x16x32_bf16 (cdna4_isa.md §10):
//   lane l holds A[row = l%16][k = (l/16)*8 + j], j = 0..7  (one b128 read)
//   B operand: lane l holds B[k = (l/16)*8 + j][col = l%16], which equals
//   Bt[col][k] — so Bt rows load with the SAME pattern as A rows.
//   C/D: lane l, reg r -> row = (l/16)*4 + r, col = l%16.
// Verified transpose-safe on hardware by tests/test_gpu_mfma.py against
// torch.matmul / MIOpen conv on asymmetric inputs.

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <initializer_list>
#include <type_traits>

namespace dwtmm {

using bf16 = c10::BFloat16;
typedef __attribute__((ext_vector_type(8))) short short8;   // bf16 x8 frag
typedef __attribute__((ext_vector_type(4))) float floatx4;  // fp32 x4 acc

#define DEV_INLINE __device__ __forceinline__

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int THREADS = 256;                // 4 waves: 2x2 of 64x64
constexpr int PAD_HALFS = 8;                // +16 B per LDS row
constexpr int LDS_PITCH = BK + PAD_HALFS;   // halves (bf16 units)
constexpr int TILE_HALFS = BM * LDS_PITCH;  // one padded operand tile
constexpr int C_PITCH = BN + PAD_HALFS;     // C staging row pitch (halves)
static_assert(BM == BN, "A and B tiles share TILE_HALFS");
static_assert(BM * C_PITCH <= 2 * TILE_HALFS,
              "C staging must fit the A/B storage");

struct ConvParams {
  int N, H, W, Cin;      // input
  int P, Q, Cout;        // output spatial + channels
  int KH, KW, stride, pad;
  int64_t M;             // N*P*Q (fwd) / N*H*W (dgrad)
  int K;                 // KH*KW*Cin (fwd) / KH*KW*Cdy (dgrad)
  int Cdy;               // dgrad: channels of dy
  int cShift = -1;       // log2 of the K-fastest channel dim if pow2
};

DEV_INLINE float bf16_to_f(unsigned short u) {
  union { unsigned int i; float f; } v;
  v.i = (unsigned int)u << 16;
  return v.f;
}
DEV_INLINE unsigned short f_to_bf16(float f) {
  union { unsigned int i; float f2; } v;
  v.f2 = f;
  unsigned int lsb = (v.i >> 16) & 1u;
  return (unsigned short)((v.i + 0x7fffu + lsb) >> 16);
}

// Tile staging, split into LOAD (issue global reads into registers, early)
// and WRITE (LDS store, late) so HBM latency hides under the MFMA phase
// (guide §6 G15 async-STAGE split / T14).  Each thread moves 32 halves as 4
// chunks of 8; a chunk-of-8 stays within one (r,s) patch element when
// Cin % 8 == 0.
struct StageRegs {
  uint4 c[4];
};

// A-operand gather modes
enum AMode { A_DENSE = 0, A_CONV = 1, A_DGRAD = 2 };

// Per-tile row cache: each thread's 4 chunk rows keep the same output
// position m across the whole K loop, so the m -> (n, p, q) decode (two
// 64-bit div/mod chains) runs ONCE per tile instead of once per k-step.
struct RowCache {
  int h0[4], w0[4];     // A_CONV: p*stride-pad / q*stride-pad; A_DGRAD: h+pad
  int64_t base[4];      // image base offset (elements)
  bool valid[4];
};

template <int MODE>
DEV_INLINE RowCache make_rows(const ConvParams& cp, int64_t m0) {
  RowCache rc;
  const int t = threadIdx.x;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int idx = t + c * THREADS;
    const int row = idx / (BK / 8);
    const int64_t m = m0 + row;
    rc.valid[c] = m < cp.M;
    const int64_t mm = rc.valid[c] ? m : 0;
    if (MODE == A_CONV) {
      const int q = (int)(mm % cp.Q);
      const int64_t np = mm / cp.Q;
      const int p = (int)(np % cp.P);
      const int n = (int)(np / cp.P);
      rc.h0[c] = p * cp.stride - cp.pad;
      rc.w0[c] = q * cp.stride - cp.pad;
      rc.base[c] = (int64_t)n * cp.H * cp.W * cp.Cin;
    } else if (MODE == A_DGRAD) {
      const int wi = (int)(mm % cp.W);
      const int64_t nh = mm / cp.W;
      const int hi = (int)(nh % cp.H);
      const int n = (int)(nh / cp.H);
      rc.h0[c] = hi + cp.pad;
      rc.w0[c] = wi + cp.pad;
      rc.base[c] = (int64_t)n * cp.P * cp.Q * cp.Cdy;
    } else {
      rc.h0[c] = 0; rc.w0[c] = 0;
      rc.base[c] = mm * cp.K;
    }
  }
  return rc;
}

// cShift >= 0 when the K-fastest channel count (Cin fwd / Cdy dgrad) is a
// power of two: replaces the per-chunk div/mod with shift/mask.
DEV_INLINE void split_kc(int kg, int cdim, int cshift, int& rs, int& cc) {
  if (cshift >= 0) {
    cc = kg & (cdim - 1);
    rs = kg >> cshift;
  } else {
    cc = kg % cdim;
    rs = kg / cdim;
  }
}

template <int MODE>
DEV_INLINE void load_a(const bf16* __restrict__ x, const ConvParams& cp,
                       const RowCache& rc, int k0, StageRegs& rg) {
  const int t = threadIdx.x;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int idx = t + c * THREADS;          // chunk index in tile
    const int kc = (idx % (BK / 8)) * 8;      // chunk k offset in tile
    const int kg = k0 + kc;
    if (!rc.valid[c] || kg >= cp.K) {
      rg.c[c] = make_uint4(0, 0, 0, 0);
      continue;
    }
    if (MODE == A_DENSE) {
      rg.c[c] = *reinterpret_cast<const uint4*>(x + rc.base[c] + kg);
      continue;
    }
    if (MODE == A_DGRAD) {
      // x here is dy (N,P,Q,Cdy) raw NHWC; k -> (r, s, co), co fastest.
      // dx[n,h,w,ci] needs dy[n, (h+pad-r)/stride, (w+pad-s)/stride, co].
      int rs, co;
      split_kc(kg, cp.Cdy, cp.cShift, rs, co);
      const int sx = rs % cp.KW;
      const int r = rs / cp.KW;
      const int hp = rc.h0[c] - r;
      const int wp = rc.w0[c] - sx;
      bool ok = hp >= 0 && wp >= 0 && hp % cp.stride == 0 && wp % cp.stride == 0;
      const int pp = hp / cp.stride, qq = wp / cp.stride;
      ok = ok && pp < cp.P && qq < cp.Q;
      if (!ok) {
        rg.c[c] = make_uint4(0, 0, 0, 0);
      } else if (cp.Cdy % 8 == 0) {
        rg.c[c] = *reinterpret_cast<const uint4*>(
            x + rc.base[c] + ((int64_t)pp * cp.Q + qq) * cp.Cdy + co);
      } else {
        unsigned short tmp[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int k = kg + j;
          unsigned short v = 0;
          if (k < cp.K && k / cp.Cdy == rs)
            v = *reinterpret_cast<const unsigned short*>(
                x + rc.base[c] + ((int64_t)pp * cp.Q + qq) * cp.Cdy + k % cp.Cdy);
          tmp[j] = v;
        }
        rg.c[c] = *reinterpret_cast<const uint4*>(tmp);
      }
      continue;
    }
    if (cp.Cin % 8 == 0) {
      int rs, ci;
      split_kc(kg, cp.Cin, cp.cShift, rs, ci);
      const int s = rs % cp.KW;
      const int r = rs / cp.KW;
      const int h = rc.h0[c] + r;
      const int w = rc.w0[c] + s;
      if (h < 0 || h >= cp.H || w < 0 || w >= cp.W) {
        rg.c[c] = make_uint4(0, 0, 0, 0);
      } else {
        rg.c[c] = *reinterpret_cast<const uint4*>(
            x + rc.base[c] + ((int64_t)h * cp.W + w) * cp.Cin + ci);
      }
    } else if (cp.Cin == 4) {
      // stem path (3-channel input zero-padded to 4 on the host): a chunk
      // of 8 halves = two horizontally adjacent pixels; when both are in
      // bounds on the same kernel row it is ONE 16-B load
      const int rs0 = kg >> 2;          // kg is 8-aligned -> ci = 0
      const int rs1 = rs0 + 1;
      const int s0 = rs0 % cp.KW, r0 = rs0 / cp.KW;
      const int h0 = rc.h0[c] + r0, w0 = rc.w0[c] + s0;
      const bool in0 = h0 >= 0 && h0 < cp.H && w0 >= 0 && w0 < cp.W;
      if (in0 && s0 + 1 < cp.KW && w0 + 1 < cp.W && kg + 4 < cp.K) {
        rg.c[c] = *reinterpret_cast<const uint4*>(
            x + rc.base[c] + ((int64_t)h0 * cp.W + w0) * 4);
      } else {
        uint2 lo = make_uint2(0, 0), hi = make_uint2(0, 0);
        if (in0)
          lo = *reinterpret_cast<const uint2*>(
              x + rc.base[c] + ((int64_t)h0 * cp.W + w0) * 4);
        if (kg + 4 < cp.K) {
          const int s1 = rs1 % cp.KW, r1 = rs1 / cp.KW;
          const int h1 = rc.h0[c] + r1, w1 = rc.w0[c] + s1;
          if (h1 >= 0 && h1 < cp.H && w1 >= 0 && w1 < cp.W)
            hi = *reinterpret_cast<const uint2*>(
                x + rc.base[c] + ((int64_t)h1 * cp.W + w1) * 4);
        }
        rg.c[c] = make_uint4(lo.x, lo.y, hi.x, hi.y);
      }
    } else {
      unsigned short tmp[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = kg + j;
        unsigned short v = 0;
        if (k < cp.K) {
          const int ci = k % cp.Cin;
          const int rs = k / cp.Cin;
          const int s = rs % cp.KW;
          const int r = rs / cp.KW;
          const int h = rc.h0[c] + r;
          const int w = rc.w0[c] + s;
          if (h >= 0 && h < cp.H && w >= 0 && w < cp.W)
            v = *reinterpret_cast<const unsigned short*>(
                x + rc.base[c] + ((int64_t)h * cp.W + w) * cp.Cin + ci);
        }
        tmp[j] = v;
      }
      rg.c[c] = *reinterpret_cast<const uint4*>(tmp);
    }
  }
}

DEV_INLINE void load_b(const bf16* __restrict__ wgt, int ncols, int K,
                       int n0, int k0, StageRegs& rg) {
  const int t = threadIdx.x;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int idx = t + c * THREADS;
    const int row = idx / (BK / 8);
    const int kc = (idx % (BK / 8)) * 8;
    const int n = n0 + row;
    const int kg = k0 + kc;
    if (n >= ncols || kg >= K) {
      rg.c[c] = make_uint4(0, 0, 0, 0);
    } else if (kg + 8 <= K) {
      rg.c[c] = *reinterpret_cast<const uint4*>(wgt + (int64_t)n * K + kg);
    } else {
      unsigned short tmp[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        tmp[j] = (kg + j < K)
            ? *reinterpret_cast<const unsigned short*>(wgt + (int64_t)n * K + kg + j)
            : (unsigned short)0;
      rg.c[c] = *reinterpret_cast<const uint4*>(tmp);
    }
  }
}

DEV_INLINE void write_tile(const StageRegs& rg, unsigned short* lds) {
  const int t = threadIdx.x;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int idx = t + c * THREADS;
    const int row = idx / (BK / 8);
    const int kc = (idx % (BK / 8)) * 8;
    *reinterpret_cast<uint4*>(lds + row * LDS_PITCH + kc) = rg.c[c];
  }
}

// ---------------------------------------------------------------------------
// Pieces shared by the 128x128 tile kernels (conv_gemm_tile, both stats
// kernels, dgrad_cls_kernel).
// ---------------------------------------------------------------------------

// XCD-aware bijective block remap (guide T1): consecutive logical ids share
// an XCD, so workgroups that read the same A rows go through one L2.
DEV_INLINE int xcd_remap(int bid, int nwg) {
  const int nx = 8;
  const int qq = nwg / nx, rr = nwg % nx;
  const int xcd = bid % nx, idx = bid / nx;
  return (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + idx;
}

struct LaneMap {
  int wm, wn;               // the wave's 64x64 sub-tile origin in the tile
  int frag_row, frag_koff;  // A/B fragment: row l%16, k (l/16)*8 .. +7
  int erow, ecol;           // C/D: lane l, reg r -> row (l/16)*4 + r, col l%16
};

DEV_INLINE LaneMap lane_map() {
  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  LaneMap lm;
  lm.wm = (wave / 2) * 64;
  lm.wn = (wave % 2) * 64;
  lm.frag_row = lane % 16;
  lm.frag_koff = (lane / 16) * 8;
  lm.erow = (lane / 16) * 4;
  lm.ecol = lane % 16;
  return lm;
}

DEV_INLINE void zero_acc(floatx4 (&acc)[4][4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (floatx4){0.f, 0.f, 0.f, 0.f};
}

// One BK step on the padded LDS image (row pitch LDS_PITCH): la / lb are the
// A / B tiles' row 0.
DEV_INLINE void mfma_kstep(const unsigned short* la, const unsigned short* lb,
                           const LaneMap& lm, floatx4 (&acc)[4][4]) {
#pragma unroll
  for (int ks = 0; ks < BK; ks += 32) {
    short8 afrag[4], bfrag[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      afrag[i] = *reinterpret_cast<const short8*>(
          la + (lm.wm + i * 16 + lm.frag_row) * LDS_PITCH + ks + lm.frag_koff);
      bfrag[i] = *reinterpret_cast<const short8*>(
          lb + (lm.wn + i * 16 + lm.frag_row) * LDS_PITCH + ks + lm.frag_koff);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            afrag[i], bfrag[j], acc[i][j], 0, 0, 0);
  }
}

// The register-staged K loop of one tile.  lds is [buf][a|b][TILE_HALFS], one
// buffer, or two with PIPE; load_a(k0, regs) / load_b(k0, regs) issue the
// global reads of the k-step at k0.
//
// PIPE: double-buffered LDS + issue-early/write-late staging (wins for
// long-K dense GEMMs, measured +24-34% at K>=2048); the simple
// single-buffer loop wins for short-K and for the implicit gather path
// (within-shape A/B on the R50 shapes).
//
// The simple loop always leaves its last k-step behind a barrier.  The
// pipelined loop does so only with LAST_BARRIER, for callers that go on to
// overwrite the buffers (C staging).
template <bool PIPE, bool LAST_BARRIER, class LoadA, class LoadB>
DEV_INLINE void staged_k_loop(int nk, unsigned short* lds, const LaneMap& lm,
                              floatx4 (&acc)[4][4], LoadA load_a,
                              LoadB load_b) {
  StageRegs ra, rb;
  if (PIPE) {
    load_a(0, ra);
    load_b(0, rb);
    write_tile(ra, lds);
    write_tile(rb, lds + TILE_HALFS);
    __syncthreads();
  }
  for (int t = 0; t < nk; ++t) {
    const int cur = PIPE ? (t & 1) : 0;
    unsigned short* la = lds + (2 * cur) * TILE_HALFS;
    unsigned short* lb = la + TILE_HALFS;
    if (PIPE) {
      // issue next tile's global loads now — they stay in flight under the
      // MFMA phase and are only waited for at the ds_write below
      if (t + 1 < nk) {
        load_a((t + 1) * BK, ra);
        load_b((t + 1) * BK, rb);
      }
    } else {
      load_a(t * BK, ra);
      load_b(t * BK, rb);
      write_tile(ra, la);
      write_tile(rb, lb);
      __syncthreads();
    }
    mfma_kstep(la, lb, lm, acc);
    if (!PIPE || LAST_BARRIER || t + 1 < nk)
      __syncthreads();  // everyone finished reading buf[cur] (and, a k-step
                        // ago, buf[cur^1])
    if (PIPE && t + 1 < nk) {
      write_tile(ra, lds + (2 * (cur ^ 1)) * TILE_HALFS);
      write_tile(rb, lds + (2 * (cur ^ 1) + 1) * TILE_HALFS);
      __syncthreads();
    }
  }
}

// ===========================================================================
// Direct-to-LDS main loop for the dense case: A rows of pitch K, Bt rows of
// pitch K, K % 64 == 0.  Both tiles go global -> LDS with 16-byte LDS-DMA
// loads (global_load_lds_dwordx4): no staging registers, no ds_write.
//
// LDS image.  One wave instruction writes 64 lanes x 16 B = 1 KB linearly
// from a wave-uniform base, i.e. 8 whole rows of an UNPADDED 128-byte-row
// tile; thread t's chunk q is tile chunk q*256 + t = row q*32 + t/8,
// position t%8.  A +16 B row pad is impossible in this image, so the bank-
// conflict fix is an XOR swizzle of the 16-byte chunk index: position p of
// row r holds the row's k-chunk p ^ swz(r).  The DMA destination stays
// linear; the permutation goes on the per-lane SOURCE address and, as the
// same involution, on the ds_read_b128 address of the fragment reads.
//
// Choice of swz.  A fragment read has 16 lanes reading rows r0..r0+15 (r0 a
// multiple of 16) at one k-chunk kc.  LDS has 64 4-byte banks = 16 groups of
// 16 B per 256 B, so a 128-byte row covers HALF of them: the group of
// (r, p) is (r & 1) * 8 + p.  With p = kc ^ swz(r) the 16 rows hit 16
// distinct groups iff swz takes 8 distinct values on the even rows (and on
// the odd rows): swz(r) = (r >> 1) & 7 does; r & 7 does not (rows r and
// r + 8 share a parity and a value, a 2-way conflict).
//
// Wait structure: the plain form, two LDS buffers of A|B, the loads of
// k-step t+1 issued before the MFMAs of k-step t and retired by vmcnt(0) +
// __syncthreads() once per k-step.  The MFMA instruction and the ascending-k
// order are those of the register-staged loop, so each accumulator sees the
// same sequence of operations and the results are bit-identical.
//
// An LDS-DMA load cannot zero-fill: rows past the operand's end are CLAMPED
// to its last row (never read out of bounds); the C rows / columns they
// feed are never stored and never enter a flushed statistic.
// ===========================================================================
constexpr int G_TILE = BM * BK;     // halves per operand tile (16 KB)
constexpr int G_BUF = 2 * G_TILE;   // one buffer: A tile, then B tile

DEV_INLINE int glds_swz(int row) { return (row >> 1) & 7; }

struct DenseSrc {
  const bf16* a;   // tile origins: row 0, k 0
  const bf16* b;
  int aoff[4];     // this thread's 4 chunks: clamped row * K + swizzled k-chunk
  int boff[4];
};

DEV_INLINE DenseSrc dense_src(const bf16* a, const bf16* b, int arows,
                              int brows, int K) {
  DenseSrc s;
  s.a = a;
  s.b = b;
  const int t = threadIdx.x;
  const int kc = ((t & 7) ^ glds_swz(t >> 3)) * 8;  // swz(q*32 + t/8) == swz(t/8)
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int row = q * (THREADS / 8) + (t >> 3);
    s.aoff[q] = (row < arows ? row : arows - 1) * K + kc;
    s.boff[q] = (row < brows ? row : brows - 1) * K + kc;
  }
  return s;
}

DEV_INLINE void glds16(const bf16* src, unsigned short* dst) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void*)src,
      (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
}

// k-step k0 of `s` -> buf (A tile, then B tile): 8 LDS-DMA loads per wave
DEV_INLINE void dense_issue(const DenseSrc& s, int k0, unsigned short* buf) {
  // wave-uniform destination; the hardware adds lane * 16 B
  unsigned short* wdst =
      buf + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * (64 * 8);
#pragma unroll
  for (int q = 0; q < 4; ++q)
    glds16(s.a + s.aoff[q] + k0, wdst + q * (THREADS * 8));
#pragma unroll
  for (int q = 0; q < 4; ++q)
    glds16(s.b + s.boff[q] + k0, wdst + G_TILE + q * (THREADS * 8));
}

DEV_INLINE void wait_vm0() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// Barrier that leaves LDS-DMA loads in flight: orders this wave's own LDS
// accesses only (__syncthreads() would also drain vmcnt).
DEV_INLINE void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// The K loop of one 128x128 tile.  On entry k-step 0 of `cur` is in
// buf[par], landed and behind a barrier, and buf[par ^ 1] is free.  With
// CHAIN and has_next the last k-step issues k-step 0 of `nxt` into the free
// buffer.  Returns the buffer index of the last k-step; its fragment reads
// are NOT yet behind a barrier, and the chained loads are still in flight.
template <bool CHAIN>
DEV_INLINE int dense_glds_loop(const DenseSrc& cur, const DenseSrc& nxt,
                               bool has_next, int nk, unsigned short* lds,
                               int par, int wm, int wn, floatx4 (&c)[4][4]) {
  const int lane = threadIdx.x % 64;
  const int frag_row = lane % 16;
  // element offset of this lane's row inside a fragment, and its row swizzle
  // (wm, wn and i * 16 are multiples of 16, so swz(row) == swz(frag_row))
  const int rowoff = frag_row * BK;
  const int sw = glds_swz(frag_row);
  int b = par;
  for (int t = 0; t < nk; ++t, b ^= 1) {
    if (t + 1 < nk) dense_issue(cur, (t + 1) * BK, lds + (b ^ 1) * G_BUF);
    else if (CHAIN && has_next) dense_issue(nxt, 0, lds + (b ^ 1) * G_BUF);
    const unsigned short* la = lds + b * G_BUF + rowoff;
    const unsigned short* lb = la + G_TILE;
#pragma unroll
    for (int ks = 0; ks < BK; ks += 32) {
      const int pc = (((ks >> 3) + (lane >> 4)) ^ sw) * 8;
      short8 afrag[4], bfrag[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        afrag[i] = *reinterpret_cast<const short8*>(la + (wm + i * 16) * BK + pc);
        bfrag[i] = *reinterpret_cast<const short8*>(lb + (wn + i * 16) * BK + pc);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          c[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afrag[i], bfrag[j], c[i][j], 0, 0, 0);
    }
    if (t + 1 < nk) {
      wait_vm0();        // k-step t+1 landed (this wave's share) ...
      __syncthreads();   // ... everyone's; and buf[b] is free for k-step t+2
    }
  }
  return b ^ 1;
}

// C staging slot of (row, col).  The padded image (pitch C_PITCH) overlays the
// register-staged loop's padded A/B storage.  The swizzled image is exactly
// BM * BN halves, one direct-to-LDS buffer: the fragment-layout 2-byte
// writes of one instruction cover 4 rows 4 apart x 32 B, which at an
// unpadded 256-B pitch would share 8 banks, so the 16-byte chunk index is
// XORed with 2 * ((row >> 2) & 3) — four distinct 32-B bank groups; a row's
// 16-byte reads stay one permuted 256-B row.
template <bool SWZC>
DEV_INLINE int c_slot(int row, int col) {
  if (!SWZC) return row * C_PITCH + col;
  return row * BN + ((((col >> 3) ^ (((row >> 2) & 3) << 1)) << 3) | (col & 7));
}

// Round the accumulators to bf16 IN PLACE (c then holds the stored values as
// floats) and stage the bf16 C tile at `cst`.  Plain ds_write only: an LDS
// atomic here would make the compiler drain every LDS-DMA load in flight.
template <bool SWZC>
DEV_INLINE void round_stage_tile(floatx4 (&c)[4][4], unsigned short* cst,
                                 const LaneMap& lm) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = lm.wn + j * 16 + lm.ecol;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const unsigned short u = f_to_bf16(c[i][j][r]);
        cst[c_slot<SWZC>(lm.wm + i * 16 + lm.erow + r, col)] = u;
        c[i][j][r] = bf16_to_f(u);
      }
    }
  }
}

// C tile out: 16 B per lane, 16 lanes per 256-B row
template <bool SWZC>
DEV_INLINE void store_c_tile(const unsigned short* cst, bf16* __restrict__ out,
                             int64_t m0, int n0, int64_t M, int Cout) {
#pragma unroll
  for (int q = 0; q < (BM * BN / 8) / THREADS; ++q) {
    const int idx = threadIdx.x + q * THREADS;
    const int row = idx / (BN / 8);
    const int cc = (idx % (BN / 8)) * 8;
    const int64_t m = m0 + row;
    const int n = n0 + cc;
    if (m < M && n < Cout)
      *reinterpret_cast<uint4*>(out + m * Cout + n) =
          *reinterpret_cast<const uint4*>(cst + c_slot<SWZC>(row, cc));
  }
}

// SWZ: the XCD block remap — only when the grid has several N-tiles to
// share.  PIPE: see staged_k_loop.
//
// One tile body serves two kernels.  EPI_NARROW is the training-path
// epilogue (optional bias / ReLU, 2-byte stores in the fragment layout).
// EPI_WIDE / EPI_WIDE_RES are the folded-inference epilogue: bias always,
// optional residual and ReLU, fp32 adds and ONE rounding, the C tile staged
// over the A/B LDS storage and written as 16-byte row-contiguous stores.
enum Epilogue { EPI_NARROW = 0, EPI_WIDE = 1, EPI_WIDE_RES = 2 };

// lds: [buf][a|b][TILE_HALFS], 16-byte aligned; the wide epilogues overlay
// the C tile on it from offset 0.
template <int MODE, bool RELU, bool HAS_BIAS, bool PIPE, bool SWZ, int EPI,
          bool GLDS = false>
DEV_INLINE void conv_gemm_tile(
    const bf16* __restrict__ x, const bf16* __restrict__ wgt,
    const float* __restrict__ bias, const bf16* __restrict__ res,
    bf16* __restrict__ out, const ConvParams& cp, int mtiles, int ntiles,
    unsigned short* lds) {
  const int bid = SWZ ? xcd_remap(blockIdx.x, mtiles * ntiles) : blockIdx.x;
  const int64_t m0 = (int64_t)(bid / ntiles) * BM;
  const int n0 = (bid % ntiles) * BN;
  const LaneMap lm = lane_map();
  const int nk = (cp.K + BK - 1) / BK;

  floatx4 acc[4][4];
  zero_acc(acc);

  if (GLDS) {
    // direct-to-LDS dense loop (the launcher guarantees K % BK == 0); lds is
    // 2 * G_BUF halves here
    static_assert(!GLDS || (MODE == A_DENSE && EPI != EPI_NARROW),
                  "the direct-to-LDS loop is dense and stores 16 bytes");
    const int arows = (int)(cp.M - m0 < BM ? cp.M - m0 : BM);
    const int brows = cp.Cout - n0 < BN ? cp.Cout - n0 : BN;
    const DenseSrc src = dense_src(x + m0 * cp.K, wgt + (int64_t)n0 * cp.K,
                                   arows, brows, cp.K);
    dense_issue(src, 0, lds);
    wait_vm0();
    __syncthreads();
    dense_glds_loop<false>(src, src, false, nk, lds, 0, lm.wm, lm.wn, acc);
    __syncthreads();  // the staging below overwrites the last k-step's buffer
  } else {
    const RowCache rc = make_rows<MODE>(cp, m0);
    staged_k_loop<PIPE, EPI != EPI_NARROW>(
        nk, lds, lm, acc,
        [&](int k0, StageRegs& rg) { load_a<MODE>(x, cp, rc, k0, rg); },
        [&](int k0, StageRegs& rg) {
          load_b(wgt, cp.Cout, cp.K, n0, k0, rg);
        });
  }

  if (EPI == EPI_NARROW) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t m = m0 + lm.wm + i * 16 + lm.erow + r;
        if (m >= cp.M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int n = n0 + lm.wn + j * 16 + lm.ecol;
          if (n >= cp.Cout) continue;
          float v = acc[i][j][r];
          if (HAS_BIAS) v += bias[n];
          if (RELU) v = fmaxf(v, 0.f);
          *reinterpret_cast<unsigned short*>(out + m * cp.Cout + n) = f_to_bf16(v);
        }
      }
    }
    return;
  }

  // ---- wide epilogue: the last k-step is behind a barrier ----
  if (EPI == EPI_WIDE_RES) {
    // residual tile -> staging, 16 B per lane; rows / columns outside the
    // tensor stay unread (their staging slots are never stored either)
#pragma unroll
    for (int q = 0; q < (BM * BN / 8) / THREADS; ++q) {
      const int idx = threadIdx.x + q * THREADS;
      const int row = idx / (BN / 8);
      const int cc = (idx % (BN / 8)) * 8;
      const int64_t m = m0 + row;
      const int n = n0 + cc;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (m < cp.M && n < cp.Cout)
        v = *reinterpret_cast<const uint4*>(res + m * cp.Cout + n);
      *reinterpret_cast<uint4*>(lds + row * C_PITCH + cc) = v;
    }
    __syncthreads();
  }
  // every C element has one owner lane: it reads the residual from its
  // staging slot, adds in fp32 (acc + bias, then + residual), rounds once
  // and writes the bf16 result back to the same slot
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = lm.wn + j * 16 + lm.ecol;
    const float b = (HAS_BIAS && n0 + col < cp.Cout) ? bias[n0 + col] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        unsigned short* slot =
            lds + c_slot<false>(lm.wm + i * 16 + lm.erow + r, col);
        float v = acc[i][j][r];
        if (HAS_BIAS) v += b;
        if (EPI == EPI_WIDE_RES) v += bf16_to_f(*slot);
        if (RELU) v = fmaxf(v, 0.f);
        *slot = f_to_bf16(v);
      }
    }
  }
  __syncthreads();
  store_c_tile<false>(lds, out, m0, n0, cp.M, cp.Cout);
}

// GLDS: the direct-to-LDS dense loop with the 16-byte-store epilogue (needs
// MODE == A_DENSE, K % BK == 0, Cout % 8 == 0 and 16-byte aligned operands;
// PIPE is ignored).
template <int MODE, bool RELU, bool HAS_BIAS, bool PIPE, bool SWZ,
          bool GLDS = false>
__global__ __launch_bounds__(THREADS, (PIPE || GLDS) ? 2 : 3)
void conv_implicit_gemm_kernel(
    const bf16* __restrict__ x, const bf16* __restrict__ wgt,
    const float* __restrict__ bias, bf16* __restrict__ out, ConvParams cp,
    int mtiles, int ntiles) {
  __shared__ __attribute__((aligned(16)))
  unsigned short lds[GLDS ? 2 * G_BUF : (PIPE ? 2 : 1) * 2 * TILE_HALFS];
  conv_gemm_tile<MODE, RELU, HAS_BIAS, PIPE, SWZ,
                 GLDS ? EPI_WIDE : EPI_NARROW, GLDS>(
      x, wgt, bias, nullptr, out, cp, mtiles, ntiles, lds);
}

// Folded-inference conv forward: out = bf16(relu?(acc + bias [+ res])).
// Needs Cout % 8 == 0 and 16-byte aligned out / res (checked by the caller).
template <int MODE, bool RELU, bool HAS_RES, bool PIPE, bool SWZ>
__global__ __launch_bounds__(THREADS, PIPE ? 2 : 3) void conv_fused_fwd_kernel(
    const bf16* __restrict__ x, const bf16* __restrict__ wgt,
    const float* __restrict__ bias, const bf16* __restrict__ res,
    bf16* __restrict__ out, ConvParams cp, int mtiles, int ntiles) {
  __shared__ __attribute__((aligned(16)))
  unsigned short lds[(PIPE ? 2 : 1) * 2 * TILE_HALFS];
  conv_gemm_tile<MODE, RELU, true, PIPE, SWZ,
                 HAS_RES ? EPI_WIDE_RES : EPI_WIDE>(
      x, wgt, bias, res, out, cp, mtiles, ntiles, lds);
}

// ===========================================================================
// 1x1 stride-1 conv forward with the FOLLOWING norm site's raw statistics
// taken in the epilogue: out[M,Cout] = x[M,Cin] @ w[Cout,Cin]^T (no bias, no
// ReLU) plus, per domain branch (`parts` equal row ranges of M), the fp32
// sums the stand-alone stats kernels would compute from `out` — so the norm
// site skips its stats pass (a full re-read of `out` from HBM).
//
//   STATS_BN:      acc[part][2][Cout]      sums, sums of squares
//   STATS_WHITEN4: acc[part*Cout/4+grp][4+16]  4 sums, then co-moments at
//                  [4 + i*4 + j] for j <= i (what whiten_stats_final reads)
//
// Statistics use the bf16-ROUNDED value that is stored.  In the 16x16 C
// fragment a lane holds one column (lane%16) and 4 rows per fragment, so the
// per-column sums over a tile's 16 rows-per-lane are lane-local and a
// whitening group of 4 channels is one lane quad (co-moments by quad-
// broadcast DPP).  Per-lane partials go to a small LDS accumulator
// (ds_add_f32) that lives ACROSS tiles: the kernel is persistent, each
// workgroup walks a contiguous run of M-tiles of one N-tile and issues one
// global atomic per statistic only when the run leaves a branch or ends
// (guide G12: per-tile global atomics would be ~19 M adds on 1.5 K
// addresses at l1.conv3).  The host guarantees (M/parts) % BM == 0, so a
// tile never straddles two branches.
//
// The C tile is staged through the A/B LDS storage after the K loop's last
// barrier and leaves as 16-byte row-contiguous stores (256 B per row per
// wave) instead of the 2-byte stores of the generic epilogue above.
// ===========================================================================

enum StatsKind { STATS_BN = 0, STATS_WHITEN4 = 1 };

template <int CTRL>
DEV_INLINE float quad_bcast(float v) {
  union { int i; float f; } a, b;
  a.f = v;
  b.i = __builtin_amdgcn_mov_dpp(a.i, CTRL, 0xf, 0xf, true);
  return b.f;
}

// Dense tile load for the kernel below: rows of `base` (row pitch K), zero
// beyond `nrows` / K.  off[c] = row*K + kc of this thread's chunk c.
DEV_INLINE void load_rows(const bf16* __restrict__ base, const int (&off)[4],
                          int nrows, int K, int k0, StageRegs& rg) {
  const int t = threadIdx.x;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int idx = t + c * THREADS;
    const int row = idx / (BK / 8);
    const int kc = (idx % (BK / 8)) * 8;
    if (row < nrows && k0 + kc < K)
      rg.c[c] = *reinterpret_cast<const uint4*>(base + off[c] + k0);
    else
      rg.c[c] = make_uint4(0, 0, 0, 0);
  }
}

// This lane's per-column partial statistics of the ROUNDED tile -> sacc.
template <int KIND>
DEV_INLINE void stats_tile(const floatx4 (&c)[4][4], float* sacc, int wn,
                           int ecol) {
  constexpr int NV = KIND == STATS_BN ? 2 : 5;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = wn + j * 16 + ecol;
    float s = 0.f, p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = c[i][j][r];
        s += v;
        if (KIND == STATS_BN) {
          p0 += v * v;
        } else {
          p0 += v * quad_bcast<0x00>(v);
          p1 += v * quad_bcast<0x55>(v);
          p2 += v * quad_bcast<0xAA>(v);
          p3 += v * quad_bcast<0xFF>(v);
        }
      }
    }
    if (KIND == STATS_BN) {
      atomicAdd(&sacc[col], s);
      atomicAdd(&sacc[BN + col], p0);
    } else {
      float* mine = sacc + col * NV;
      atomicAdd(&mine[0], s);
      atomicAdd(&mine[1], p0);
      atomicAdd(&mine[2], p1);
      atomicAdd(&mine[3], p2);
      atomicAdd(&mine[4], p3);
    }
  }
}

// sacc -> the global accumulator of branch `part`, and zero it
template <int KIND>
DEV_INLINE void stats_flush(float* sacc, float* __restrict__ acc, int part,
                            int n0, int Cout) {
  constexpr int NV = KIND == STATS_BN ? 2 : 5;
  for (int k = threadIdx.x; k < BN * NV; k += THREADS) {
    const float v = sacc[k];
    sacc[k] = 0.f;
    if (KIND == STATS_BN) {
      const int which = k / BN;
      const int n = n0 + k % BN;
      if (n < Cout)
        atomicAdd(acc + ((int64_t)part * 2 + which) * Cout + n, v);
    } else {
      const int n = n0 + k / NV;
      const int e = k % NV;
      const int i = n & 3;
      if (n < Cout && e <= i + 1) {
        const int64_t grp = (int64_t)part * (Cout / 4) + n / 4;
        const int slot = e == 0 ? i : 4 + i * 4 + (e - 1);
        atomicAdd(acc + grp * 20 + slot, v);
      }
    }
  }
}

template <bool PIPE, int KIND>
__global__ __launch_bounds__(THREADS, PIPE ? 2 : 3) void conv1x1_stats_kernel(
    const bf16* __restrict__ x, const bf16* __restrict__ wgt,
    bf16* __restrict__ out, float* __restrict__ acc, ConvParams cp,
    int mtiles, int ntiles, int tiles_per_part, int nlanes, int runs) {
  constexpr int NV = KIND == STATS_BN ? 2 : 5;   // LDS stats per column
  // [buf][a|b][TILE_HALFS]; the C staging tile overlays it from offset 0
  __shared__ __attribute__((aligned(16)))
  unsigned short lds[(PIPE ? 2 : 1) * 2 * TILE_HALFS];
  __shared__ float sacc[BN * NV];

  // XCD remap: the workgroups walking the same M-run for neighbouring
  // N-tiles read their A tiles through one L2
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int nlane = bid % nlanes;
  const int run = bid / nlanes;
  const int mt_begin = (int)((int64_t)run * mtiles / runs);
  const int mt_end = (int)((int64_t)(run + 1) * mtiles / runs);

  const LaneMap lm = lane_map();
  const int nk = (cp.K + BK - 1) / BK;

  // A and B tiles stage with one chunk map: element offsets row*K + kc from
  // a per-tile base pointer (32-bit, shared by both operands)
  int off[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int idx = threadIdx.x + q * THREADS;
    off[q] = (idx / (BK / 8)) * cp.K + (idx % (BK / 8)) * 8;
  }

  for (int k = threadIdx.x; k < BN * NV; k += THREADS) sacc[k] = 0.f;
  __syncthreads();

  for (int nt = nlane; nt < ntiles; nt += nlanes) {
    const int n0 = nt * BN;
    const bf16* wb = wgt + (int64_t)n0 * cp.K;
    const int brows = cp.Cout - n0 < BN ? cp.Cout - n0 : BN;
    for (int mt = mt_begin; mt < mt_end; ++mt) {
      const int64_t m0 = (int64_t)mt * BM;

      floatx4 c[4][4];
      zero_acc(c);
      const bf16* xa = x + m0 * cp.K;
      const int arows = (int)(cp.M - m0 < BM ? cp.M - m0 : BM);
      // the last k-step ends on a barrier: the C staging below overwrites
      // both buffers
      staged_k_loop<PIPE, true>(
          nk, lds, lm, c,
          [&](int k0, StageRegs& rg) { load_rows(xa, off, arows, cp.K, k0, rg); },
          [&](int k0, StageRegs& rg) { load_rows(wb, off, brows, cp.K, k0, rg); });

      // ---- epilogue: round, stage C in LDS, per-column statistics ----
      // rows m >= M and columns n >= Cout hold exact zeros (their A / B
      // rows were zero-filled), so they add nothing to the sums
      round_stage_tile<false>(c, lds, lm);
      stats_tile<KIND>(c, sacc, lm.wn, lm.ecol);
      __syncthreads();
      store_c_tile<false>(lds, out, m0, n0, cp.M, cp.Cout);
      __syncthreads();  // staging free again; this tile's sacc adds visible

      // ---- flush when the run leaves this branch or ends ----
      const int part = mt / tiles_per_part;
      if (mt + 1 == mt_end || (mt + 1) / tiles_per_part != part) {
        stats_flush<KIND>(sacc, acc, part, n0, cp.Cout);
        __syncthreads();
      }
    }
  }
}

// The same kernel on the direct-to-LDS loop (K % BK == 0), with cross-tile
// prefetch: a workgroup's tiles form one sequence (its M-run for each of its
// N-tiles in turn) and the last k-step of a tile issues k-step 0 of the NEXT
// tile into the free buffer, so those loads fly under the rounding, the
// statistics, the C staging and the start of the stores.  The buffer parity
// carries from tile to tile.  All LDS is one array: [2][A|B] then sacc.
//
// Epilogue order, and why each barrier is there (buffer L = the last k-step's,
// buffer F = the one the chained loads fill):
//   lds_barrier        every wave finished its fragment reads of L; the
//                      chained loads stay in flight (no vmcnt wait)
//   round, stage C in L (swizzled, exactly one buffer, so it cannot touch
//                      F); no statistics yet (an LDS atomic here would drain
//                      the chained loads)
//   vmcnt(0) + __syncthreads   C staging visible; the chained loads retired
//                      before any global store is issued, so the wait covers
//                      loads only, and the next tile's first fragment read of
//                      F is behind this wait and barrier
//   C read from L -> 16-byte global stores; statistics of the rounded
//                      values -> sacc; [lds_barrier; flush]
//   lds_barrier        C reads of L and the flush's sacc zeroing are done
//                      before the next tile's k-step 1 loads land in L / its
//                      epilogue adds to sacc; the stores stay in flight
template <int KIND>
__global__ __launch_bounds__(THREADS, 2) void conv1x1_stats_glds_kernel(
    const bf16* __restrict__ x, const bf16* __restrict__ wgt,
    bf16* __restrict__ out, float* __restrict__ acc, ConvParams cp,
    int mtiles, int ntiles, int tiles_per_part, int nlanes, int runs) {
  constexpr int NV = KIND == STATS_BN ? 2 : 5;   // LDS stats per column
  __shared__ __attribute__((aligned(16)))
  unsigned short lds[2 * G_BUF + BN * NV * 2];
  float* sacc = reinterpret_cast<float*>(lds + 2 * G_BUF);
  static_assert(BM * BN <= G_BUF, "C staging must fit one buffer");

  // XCD remap and run split: as conv1x1_stats_kernel
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int nlane = bid % nlanes;
  const int run = bid / nlanes;
  const int mt_begin = (int)((int64_t)run * mtiles / runs);
  const int mt_end = (int)((int64_t)(run + 1) * mtiles / runs);

  const LaneMap lm = lane_map();
  const int nk = cp.K / BK;

  for (int k = threadIdx.x; k < BN * NV; k += THREADS) sacc[k] = 0.f;

  // the host guarantees M % BM == 0, so every A tile is whole
  auto tile_src = [&](int nt, int mt) {
    const int n0 = nt * BN;
    return dense_src(x + (int64_t)mt * BM * cp.K, wgt + (int64_t)n0 * cp.K, BM,
                     cp.Cout - n0 < BN ? cp.Cout - n0 : BN, cp.K);
  };

  int nt = nlane, mt = mt_begin;   // nlanes <= ntiles and runs <= mtiles
  DenseSrc cur = tile_src(nt, mt);
  dense_issue(cur, 0, lds);
  wait_vm0();
  __syncthreads();                 // also publishes the zeroed sacc
  int par = 0;
  for (;;) {
    int nmt = mt + 1, nnt = nt;
    if (nmt == mt_end) { nmt = mt_begin; nnt = nt + nlanes; }
    const bool has_next = nnt < ntiles;
    const DenseSrc nxt = has_next ? tile_src(nnt, nmt) : cur;

    floatx4 c[4][4];
    zero_acc(c);
    const int last = dense_glds_loop<true>(cur, nxt, has_next, nk, lds, par,
                                           lm.wm, lm.wn, c);
    unsigned short* cst = lds + last * G_BUF;

    lds_barrier();
    // columns n >= Cout were computed from a clamped B row: never stored,
    // and the flush below drops their sums
    round_stage_tile<true>(c, cst, lm);
    wait_vm0();
    __syncthreads();
    const int n0 = nt * BN;
    store_c_tile<true>(cst, out, (int64_t)mt * BM, n0, cp.M, cp.Cout);
    stats_tile<KIND>(c, sacc, lm.wn, lm.ecol);
    const int part = mt / tiles_per_part;
    if (mt + 1 == mt_end || (mt + 1) / tiles_per_part != part) {
      lds_barrier();   // every wave's sacc adds are in
      stats_flush<KIND>(sacc, acc, part, n0, cp.Cout);
    }
    lds_barrier();

    if (!has_next) break;
    cur = nxt;
    nt = nnt;
    mt = nmt;
    par = last ^ 1;
  }
}

// ===========================================================================
// wgrad v2: dw[co][(r,s,ci)] = sum_{k=npq} dy[k][co] * xpatch[k][(r,s,ci)]
//
// The K dimension is the (huge) output-position axis, so the kernel is
// SPLIT-K: the grid is (mtiles * ntiles * splitk) and each block accumulates
// its K-slab into an fp32 workspace with atomicAdd; a tiny convert kernel
// writes the bf16 dw afterwards.  Both operands are K-major with stride C
// in memory, so tiles are loaded coalesced in (k, c) orientation and
// TRANSPOSED through LDS into the (c, k) fragment layout the MFMA wants.
// 64x64 tile, BK=64, 4 waves each doing a 32x32 quadrant.
//
// B (x patches): when Cin % 64 == 0 every 64-column N-tile lies inside one
// (r, s) tap, so the gather is one shifted NHWC base + coalesced 16-B
// chunks; otherwise (stem Cin=3) a scalar per-element gather.
// ===========================================================================



constexpr int WBK = 64;
constexpr int WPITCH = WBK;  // no pad: the chunk XOR swizzle below spreads
                             // banks instead

// LDS transpose swizzle: element (row, k) lives at
//   row*WPITCH + ((k>>3) ^ wswz(row))*8 + (k&7)
// wswz varies with BOTH row%8 and row/8, so the transpose's strided stores
// (8 rows x one k-pair per wave instruction) spread across all banks
// (un-swizzled they land 16-way conflicted), while b128 fragment reads of
// 8-aligned k-chunks stay contiguous.
DEV_INLINE int wswz(int row) { return ((row >> 3) ^ row) & 7; }

// WT = square tile side (64 for small Cout/RSC shapes, 128 otherwise —
// the 64 tile re-reads operands across tiles and goes HBM-bound on big
// shapes; the 128 tile wastes MFMA work when M or N < 128).
template <bool ALIGNED_B, int WT>
__global__ __launch_bounds__(256, WT == 64 ? 4 : 3) void wgrad_splitk_kernel(
    const bf16* __restrict__ dy, const bf16* __restrict__ x,
    float* __restrict__ ws, ConvParams cp, int mtiles, int ntiles,
    int splitk, int64_t klen) {
  constexpr int NP = WT / 64;   // load passes per operand
  constexpr int NF = WT / 32;   // MFMA fragments per wave dim
  __shared__ unsigned short lds_a[WT * WPITCH];  // [co][k]
  __shared__ unsigned short lds_b[WT * WPITCH];  // [rsci][k]

  const int bid = blockIdx.x;
  const int tile = bid / splitk;
  const int kchunk = bid % splitk;
  const int m0 = (tile / ntiles) * WT;   // co origin
  const int n0 = (tile % ntiles) * WT;   // rsci origin
  const int64_t ks = (int64_t)kchunk * klen;
  const int64_t ke = (ks + klen < cp.M) ? ks + klen : cp.M;  // cp.M = real NPQ

  const int t = threadIdx.x;
  const int wave = t / 64;
  const int lane = t % 64;
  const int wm = (wave / 2) * (WT / 2);
  const int wn = (wave % 2) * (WT / 2);

  floatx4 acc[NF][NF];
#pragma unroll
  for (int i = 0; i < NF; ++i)
#pragma unroll
    for (int j = 0; j < NF; ++j) acc[i][j] = (floatx4){0.f, 0.f, 0.f, 0.f};

  const int frag_row = lane % 16;
  const int frag_koff = (lane / 16) * 8;

  // thread t owns channel chunk (t%8)*8 (two 64-row passes) and the k-pair
  // 2*(t/8): adjacent k values pack into ds_write_b32 (per-element u16
  // transpose stores cost 4x the LDS write cycles)
  const int cch = (t % 8) * 8;
  const int kp = 2 * (t / 8);

  for (int64_t k0 = ks; k0 < ke; k0 += WBK) {
    const int64_t ka = k0 + kp;
    // ---- dy tile [WBK k][WT co] -> lds_a[co][k] ----
#pragma unroll
    for (int pass = 0; pass < NP; ++pass) {
      const int c2 = cch + pass * 64;
      uint4 u0 = make_uint4(0, 0, 0, 0), u1 = make_uint4(0, 0, 0, 0);
      if (m0 + c2 < cp.N) {  // cp.N = Cout here
        if (ka < ke)
          u0 = *reinterpret_cast<const uint4*>(dy + ka * cp.N + m0 + c2);
        if (ka + 1 < ke)
          u1 = *reinterpret_cast<const uint4*>(dy + (ka + 1) * cp.N + m0 + c2);
      }
      const unsigned short* v0 = reinterpret_cast<const unsigned short*>(&u0);
      const unsigned short* v1 = reinterpret_cast<const unsigned short*>(&u1);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int row = c2 + j;
        const unsigned int pk = (unsigned int)v0[j] | ((unsigned int)v1[j] << 16);
        *reinterpret_cast<unsigned int*>(
            lds_a + row * WPITCH + (((kp >> 3) ^ wswz(row)) << 3) + (kp & 7)) = pk;
      }
    }
    // ---- x-patch tile [WBK k][WT rsci] -> lds_b[rsci][k] ----
#pragma unroll
    for (int pass = 0; pass < NP; ++pass) {
      const int c2 = cch + pass * 64;
      unsigned short v0[8], v1[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { v0[j] = 0; v1[j] = 0; }
      // when Cin % 64 == 0 the 8-row chunk (64-aligned) sits in ONE tap
      int rB = 0, sB = 0, ciB = 0;
      if (ALIGNED_B) {
        const int rs = (n0 + c2) / cp.Cin;
        sB = rs % cp.KW;
        rB = rs / cp.KW;
        ciB = (n0 + c2) % cp.Cin;
      }
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int64_t k = ka + half;
        unsigned short* v = half ? v1 : v0;
        if (k >= ke) continue;
        const int q = (int)(k % cp.Q);
        const int64_t np = k / cp.Q;
        const int p = (int)(np % cp.P);
        const int n = (int)(np / cp.P);
        if (ALIGNED_B) {
          const int h = p * cp.stride - cp.pad + rB;
          const int w = q * cp.stride - cp.pad + sB;
          if (h >= 0 && h < cp.H && w >= 0 && w < cp.W)
            *reinterpret_cast<uint4*>(v) = *reinterpret_cast<const uint4*>(
                x + (((int64_t)n * cp.H + h) * cp.W + w) * cp.Cin + ciB);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int nr = n0 + c2 + j;
            if (nr >= cp.Cout) break;   // cp.Cout = KH*KW*Cin columns
            const int ci = nr % cp.Cin;
            const int rs = nr / cp.Cin;
            const int sx = rs % cp.KW;
            const int r = rs / cp.KW;
            const int h = p * cp.stride - cp.pad + r;
            const int w = q * cp.stride - cp.pad + sx;
            if (h >= 0 && h < cp.H && w >= 0 && w < cp.W)
              v[j] = *reinterpret_cast<const unsigned short*>(
                  x + (((int64_t)n * cp.H + h) * cp.W + w) * cp.Cin + ci);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int row = c2 + j;
        const unsigned int pk = (unsigned int)v0[j] | ((unsigned int)v1[j] << 16);
        *reinterpret_cast<unsigned int*>(
            lds_b + row * WPITCH + (((kp >> 3) ^ wswz(row)) << 3) + (kp & 7)) = pk;
      }
    }
    __syncthreads();
#pragma unroll
    for (int kstep = 0; kstep < WBK; kstep += 32) {
      short8 afrag[NF], bfrag[NF];
      const int kb = (kstep + frag_koff) >> 3;  // 8-aligned chunk index
#pragma unroll
      for (int i = 0; i < NF; ++i) {
        const int ra = wm + i * 16 + frag_row;
        const int rb = wn + i * 16 + frag_row;
        afrag[i] = *reinterpret_cast<const short8*>(
            lds_a + ra * WPITCH + ((kb ^ wswz(ra)) << 3));
        bfrag[i] = *reinterpret_cast<const short8*>(
            lds_b + rb * WPITCH + ((kb ^ wswz(rb)) << 3));
      }
#pragma unroll
      for (int i = 0; i < NF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afrag[i], bfrag[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }

  // epilogue: atomicAdd fp32 workspace [Cout][RSC]
  const int erow = (lane / 16) * 4;
  const int ecol = lane % 16;
#pragma unroll
  for (int i = 0; i < NF; ++i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + wm + i * 16 + erow + r;
      if (m >= cp.N) continue;
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        const int n = n0 + wn + j * 16 + ecol;
        if (n >= cp.Cout) continue;
        atomicAdd(&ws[(int64_t)m * cp.Cout + n], acc[i][j][r]);
      }
    }
  }
}

__global__ void f32_to_bf16_kernel(const float* __restrict__ src,
                                   bf16* __restrict__ dst, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    *reinterpret_cast<unsigned short*>(dst + i) = f_to_bf16(src[i]);
}

// ===========================================================================
// Class-decomposed strided dgrad.  For stride s, dx positions split into s*s
// residue classes (h%s, w%s); each class has a FIXED subset of (r,s) taps
// that satisfy the stride-divisibility, so the per-class GEMM runs only the
// useful K (ntaps*Cdy) instead of wading through KH*KW*Cdy that is ~3/4
// zeros (the single-kernel gather measured 0.13-0.22x library on the R50
// stride-2 shapes).  One launch per class; 128x128 tile as the main kernel.
// ===========================================================================

struct DgradClsParams {
  int H, W, Cin, P, Q, Cdy, Kfull;  // Kfull = KH*KW*Cdy (wd row pitch)
  int ch, cw, stride;
  int Hc, Wc;              // class spatial extent
  int64_t M;               // N*Hc*Wc
  int K;                   // ntaps*Cdy
  int cShift;              // log2(Cdy), Cdy % 8 == 0 guaranteed
  int dp[16], dq[16], rsIdx[16];
};

__global__ __launch_bounds__(THREADS, 3) void dgrad_cls_kernel(
    const bf16* __restrict__ dy, const bf16* __restrict__ wd,
    bf16* __restrict__ dx, DgradClsParams gp, int mtiles, int ntiles) {
  __shared__ unsigned short lds_a[BM * LDS_PITCH];
  __shared__ unsigned short lds_b[BN * LDS_PITCH];
  const int bid = blockIdx.x;
  const int64_t m0 = (int64_t)(bid / ntiles) * BM;
  const int n0 = (bid % ntiles) * BN;
  const LaneMap lm = lane_map();

  floatx4 acc[4][4];
  zero_acc(acc);

  // row cache: class position m -> (n, hh, ww)
  int rcP[4], rcQ[4];
  int64_t rbase[4];
  bool rvalid[4];
  {
    const int t = threadIdx.x;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int idx = t + c * THREADS;
      const int row = idx / (BK / 8);
      const int64_t m = m0 + row;
      rvalid[c] = m < gp.M;
      const int64_t mm = rvalid[c] ? m : 0;
      const int ww = (int)(mm % gp.Wc);
      const int64_t nh = mm / gp.Wc;
      const int hh = (int)(nh % gp.Hc);
      const int n = (int)(nh / gp.Hc);
      rcP[c] = hh;
      rcQ[c] = ww;
      rbase[c] = (int64_t)n * gp.P * gp.Q * gp.Cdy;
    }
  }

  const int nk = (gp.K + BK - 1) / BK;
  const int t = threadIdx.x;

  for (int kt = 0; kt < nk; ++kt) {
    const int k0 = kt * BK;
    // A: dy gather
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int idx = t + c * THREADS;
      const int kc = (idx % (BK / 8)) * 8;
      const int kg = k0 + kc;
      uint4 val = make_uint4(0, 0, 0, 0);
      if (rvalid[c] && kg < gp.K) {
        const int tap = kg >> gp.cShift;
        const int co = kg & (gp.Cdy - 1);
        const int pp = rcP[c] + gp.dp[tap];
        const int qq = rcQ[c] + gp.dq[tap];
        if (pp >= 0 && pp < gp.P && qq >= 0 && qq < gp.Q)
          val = *reinterpret_cast<const uint4*>(
              dy + rbase[c] + ((int64_t)pp * gp.Q + qq) * gp.Cdy + co);
      }
      const int row = (t + c * THREADS) / (BK / 8);
      *reinterpret_cast<uint4*>(lds_a + row * LDS_PITCH + kc) = val;
    }
    // B: wd rows (ci), k -> (tap, co) -> wd[n][rsIdx[tap]*Cdy + co]
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int idx = t + c * THREADS;
      const int row = idx / (BK / 8);
      const int kc = (idx % (BK / 8)) * 8;
      const int kg = k0 + kc;
      const int n = n0 + row;
      uint4 val = make_uint4(0, 0, 0, 0);
      if (n < gp.Cin && kg < gp.K) {
        const int tap = kg >> gp.cShift;
        const int co = kg & (gp.Cdy - 1);
        val = *reinterpret_cast<const uint4*>(
            wd + (int64_t)n * gp.Kfull + gp.rsIdx[tap] * gp.Cdy + co);
      }
      *reinterpret_cast<uint4*>(lds_b + row * LDS_PITCH + kc) = val;
    }
    __syncthreads();
    mfma_kstep(lds_a, lds_b, lm, acc);
    __syncthreads();
  }

  // epilogue: scatter to dx[n, hh*s+ch, ww*s+cw, ci]
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t m = m0 + lm.wm + i * 16 + lm.erow + r;
      if (m >= gp.M) continue;
      const int ww = (int)(m % gp.Wc);
      const int64_t nh = m / gp.Wc;
      const int hh = (int)(nh % gp.Hc);
      const int n = (int)(nh / gp.Hc);
      const int h = hh * gp.stride + gp.ch;
      const int w = ww * gp.stride + gp.cw;
      const int64_t obase = (((int64_t)n * gp.H + h) * gp.W + w) * gp.Cin;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = n0 + lm.wn + j * 16 + lm.ecol;
        if (col >= gp.Cin) continue;
        *reinterpret_cast<unsigned short*>(dx + obase + col) =
            f_to_bf16(acc[i][j][r]);
      }
    }
  }
}

}  // namespace dwtmm

// ---------------------------------------------------------------------------
// launchers (referenced from dwt_kernels.hip bindings)
// ---------------------------------------------------------------------------

using torch::Tensor;

static inline hipStream_t dwtmm_stream() {
  return at::cuda::getCurrentCUDAStream().stream();
}

static inline int log2_if_pow2(int64_t v) {
  return (v > 0 && (v & (v - 1)) == 0) ? __builtin_ctzll((uint64_t)v) : -1;
}

// ---- runtime values -> template arguments --------------------------------
// static_dispatch(f, a, b, ...) calls the generic lambda f with one
// std::integral_constant per argument: a bool arrives as std::true_type /
// std::false_type, a OneOf<V0, V1, ...>{v} as the integral_constant<int, Vi>
// with Vi == v.  f is instantiated for every combination, so pass only what
// can vary at the call site.
template <int... Vs>
struct OneOf { int64_t v; };

template <class F>
static void static_dispatch(F&& f) { f(); }

template <class F, int V0, int... Vs, class... Rest>
static void static_dispatch(F&& f, OneOf<V0, Vs...> e, Rest... rest);

template <class F, class... Rest>
static void static_dispatch(F&& f, bool b, Rest... rest) {
  auto bind = [&](auto c) {
    static_dispatch([&](auto... cs) { f(c, cs...); }, rest...);
  };
  if (b) bind(std::true_type{});
  else bind(std::false_type{});
}

template <class F, int V0, int... Vs, class... Rest>
static void static_dispatch(F&& f, OneOf<V0, Vs...> e, Rest... rest) {
  if (e.v == V0) {
    static_dispatch(
        [&](auto... cs) { f(std::integral_constant<int, V0>{}, cs...); },
        rest...);
    return;
  }
  if constexpr (sizeof...(Vs) > 0)
    static_dispatch(f, OneOf<Vs...>{e.v}, rest...);
  else
    TORCH_CHECK(false, "static_dispatch: no instantiation for value ", e.v);
}

// ---- argument checks, ConvParams and the tile plan ------------------------

struct Operand {
  const char* name;
  const Tensor& t;
  at::ScalarType dtype;
  int64_t numel;   // what the passed geometry says
};

static void check_operands(const char* who,
                           std::initializer_list<Operand> ops) {
  for (const Operand& o : ops)
    TORCH_CHECK(o.t.defined() && o.t.is_cuda() &&
                    o.t.scalar_type() == o.dtype && o.t.numel() == o.numel,
                who, ": ", o.name, " must be a ", o.dtype, " GPU tensor of ",
                o.numel, " elements");
}

// C[M,N] = A[M,K] @ Bt[N,K]^T
static dwtmm::ConvParams gemm_params(const char* who, int64_t M, int64_t K,
                                     int64_t N) {
  TORCH_CHECK(M > 0 && N > 0 && K >= 0 && K <= INT_MAX && N <= INT_MAX, who,
              ": GEMM extents ", M, " x ", K, " x ", N);
  dwtmm::ConvParams cp{};
  cp.M = M; cp.K = (int)K; cp.Cout = (int)N;
  return cp;
}

// Conv geometry as the entry points receive it.  For dgrad, Cout is Cdy.
struct ConvGeom {
  int64_t N, H, W, Cin, P, Q, Cout, KH, KW, stride, pad;
  // a plain GEMM over the positions
  bool unit() const { return KH == 1 && KW == 1 && stride == 1 && pad == 0; }
};

// fwd: M = N*P*Q rows of K = KH*KW*Cin, Cout columns.  dgrad: M = N*H*W rows
// of K = KH*KW*Cdy, Cin columns.
static dwtmm::ConvParams conv_params(const char* who, const ConvGeom& g,
                                     bool dgrad) {
  TORCH_CHECK(g.N > 0 && g.H > 0 && g.W > 0 && g.Cin > 0 && g.P > 0 &&
                  g.Q > 0 && g.Cout > 0 && g.KH > 0 && g.KW > 0 &&
                  g.stride > 0 && g.pad >= 0,
              who, ": conv geometry");
  const int64_t cfast = dgrad ? g.Cout : g.Cin;   // the K-fastest channels
  dwtmm::ConvParams cp =
      gemm_params(who, dgrad ? g.N * g.H * g.W : g.N * g.P * g.Q,
                  g.KH * g.KW * cfast, dgrad ? g.Cin : g.Cout);
  cp.N = g.N; cp.H = g.H; cp.W = g.W; cp.Cin = g.Cin;
  cp.P = g.P; cp.Q = g.Q;
  cp.KH = g.KH; cp.KW = g.KW; cp.stride = g.stride; cp.pad = g.pad;
  cp.Cdy = dgrad ? g.Cout : 0;
  cp.cShift = log2_if_pow2(cfast);
  return cp;
}

struct TilePlan {
  int mtiles, ntiles;
  bool gemm_fast;   // the A operand is a dense [M, K] matrix (A_DENSE)
  bool pipe, swz;   // PIPE / SWZ of the tile kernels
};

// unit: 1x1 stride-1 pad-0 geometry; cfast: the K-fastest channel count.
static TilePlan tile_plan(const char* who, const dwtmm::ConvParams& cp,
                          bool unit, int64_t cfast) {
  const int64_t mt = (cp.M + dwtmm::BM - 1) / dwtmm::BM;
  const int64_t nt = (cp.Cout + dwtmm::BN - 1) / dwtmm::BN;
  TORCH_CHECK(mt * nt < (int64_t)1 << 31, who, ": grid of ", mt, " x ", nt,
              " tiles does not fit 32 bits");
  TilePlan tp;
  tp.mtiles = (int)mt;
  tp.ntiles = (int)nt;
  tp.gemm_fast = unit && cfast % 8 == 0;
  // pipelined staging pays only on the dense path (measured: the gather
  // path's extra register pressure under PIPE regressed l3.conv2 0.91->0.60)
  tp.pipe = tp.gemm_fast && cp.K >= 4 * dwtmm::BK;
  tp.swz = tp.gemm_fast && nt >= 8 && mt * nt >= 16;
  return tp;
}

// ---- the direct-to-LDS switch ---------------------------------------------
// The dense kernels take the direct-to-LDS loop where it applies unless this
// is off (DWT_AMD_DENSE_GLDS=0 through dispatch, or set_dense_glds()).
static bool g_dense_glds = true;
static int64_t g_dense_glds_launches = 0;

void set_dense_glds(bool on) { g_dense_glds = on; }
bool dense_glds_selected() { return g_dense_glds; }
// launches that took the direct-to-LDS loop since the extension was loaded
int64_t dense_glds_launches() { return g_dense_glds_launches; }

static inline bool aligned16(const Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

// Whether a dense GEMM A[M,K] @ Bt[N,K]^T -> out[M,N] can run on the
// direct-to-LDS loop: whole k-steps (an LDS-DMA load cannot zero-fill), 16-byte
// loads of both operands and 16-byte stores of the output.
static inline bool dense_glds_ok(const Tensor& a, const Tensor& bt,
                                 const Tensor& out,
                                 const dwtmm::ConvParams& cp) {
  return g_dense_glds && cp.K > 0 && cp.K % dwtmm::BK == 0 &&
         cp.Cout % 8 == 0 && aligned16(a) && aligned16(bt) && aligned16(out);
}

using ADense = std::integral_constant<int, dwtmm::A_DENSE>;
using AConv = std::integral_constant<int, dwtmm::A_CONV>;
using ADgrad = std::integral_constant<int, dwtmm::A_DGRAD>;
constexpr std::false_type kOff{};

// conv_implicit_gemm_kernel, instantiated for what tile_plan can select:
//   A_DENSE x {RELU, BIAS, PIPE, SWZ}, and on the direct-to-LDS loop
//   x {RELU, BIAS, SWZ};  A_CONV x {RELU, BIAS};  A_DGRAD.
// mode is A_CONV / A_DGRAD for the gather; tp.gemm_fast overrides it.
static void launch_conv_gemm(int mode, const Tensor& a, const Tensor& bt,
                             const float* bias, const Tensor& out,
                             const dwtmm::ConvParams& cp, const TilePlan& tp,
                             bool relu) {
  auto go = [&](auto modec, auto reluc, auto biasc, auto pipec, auto swzc,
                auto gldsc) {
    hipLaunchKernelGGL(
        (dwtmm::conv_implicit_gemm_kernel<
            decltype(modec)::value, decltype(reluc)::value,
            decltype(biasc)::value, decltype(pipec)::value,
            decltype(swzc)::value, decltype(gldsc)::value>),
        dim3(tp.mtiles * tp.ntiles), dim3(dwtmm::THREADS), 0, dwtmm_stream(),
        (const c10::BFloat16*)a.data_ptr(), (const c10::BFloat16*)bt.data_ptr(),
        bias, (c10::BFloat16*)out.data_ptr(), cp, tp.mtiles, tp.ntiles);
  };
  const bool has_bias = bias != nullptr;
  if (tp.gemm_fast && dense_glds_ok(a, bt, out, cp)) {
    static_dispatch(
        [&](auto r, auto b, auto z) { go(ADense{}, r, b, kOff, z, std::true_type{}); },
        relu, has_bias, tp.swz);
    ++g_dense_glds_launches;
  } else if (tp.gemm_fast) {
    static_dispatch(
        [&](auto r, auto b, auto p, auto z) { go(ADense{}, r, b, p, z, kOff); },
        relu, has_bias, tp.pipe, tp.swz);
  } else if (mode == dwtmm::A_CONV) {
    static_dispatch(
        [&](auto r, auto b) { go(AConv{}, r, b, kOff, kOff, kOff); }, relu,
        has_bias);
  } else {
    TORCH_CHECK(mode == dwtmm::A_DGRAD && !relu && !has_bias,
                "launch_conv_gemm: no such instantiation");
    go(ADgrad{}, kOff, kOff, kOff, kOff, kOff);
  }
}

static const float* bias_ptr(const char* who, const Tensor& bias,
                             bool has_bias, int64_t n) {
  if (!has_bias) return nullptr;
  check_operands(who, {{"bias", bias, at::kFloat, n}});
  return bias.data_ptr<float>();
}

// C[M,N] = A[M,K] @ Bt[N,K]^T (+bias +relu), all bf16, fp32 accumulate.
// K % 8 == 0 (the A rows load 16 bytes at a time).
void mfma_gemm(Tensor a, Tensor bt, Tensor bias, Tensor out, bool relu,
               bool has_bias) {
  const char* who = "mfma_gemm";
  TORCH_CHECK(a.dim() == 2 && bt.dim() == 2, who, ": a and bt must be 2-D");
  const int64_t M = a.size(0), K = a.size(1), N = bt.size(0);
  TORCH_CHECK(bt.size(1) == K && K % 8 == 0, who, ": K = ", K);
  check_operands(who, {{"a", a, at::kBFloat16, M * K},
                       {"bt", bt, at::kBFloat16, N * K},
                       {"out", out, at::kBFloat16, M * N}});
  const dwtmm::ConvParams cp = gemm_params(who, M, K, N);
  launch_conv_gemm(dwtmm::A_DENSE, a, bt, bias_ptr(who, bias, has_bias, N),
                   out, cp, tile_plan(who, cp, true, K), relu);
}

// NHWC conv fwd: x (N,H,W,Cin) raw storage, wgt (Cout, KH*KW*Cin) raw
// channels_last storage, out (N,P,Q,Cout) raw storage.
void mfma_conv2d_fwd(Tensor x, Tensor wgt, Tensor bias, Tensor out,
                     int64_t N, int64_t H, int64_t W, int64_t Cin,
                     int64_t P, int64_t Q, int64_t Cout, int64_t KH,
                     int64_t KW, int64_t stride, int64_t pad, bool relu,
                     bool has_bias) {
  const char* who = "mfma_conv2d_fwd";
  const ConvGeom g{N, H, W, Cin, P, Q, Cout, KH, KW, stride, pad};
  const dwtmm::ConvParams cp = conv_params(who, g, false);
  check_operands(who, {{"x", x, at::kBFloat16, N * H * W * Cin},
                       {"wgt", wgt, at::kBFloat16, Cout * cp.K},
                       {"out", out, at::kBFloat16, cp.M * Cout}});
  launch_conv_gemm(dwtmm::A_CONV, x, wgt, bias_ptr(who, bias, has_bias, Cout),
                   out, cp, tile_plan(who, cp, g.unit(), Cin), relu);
}

// Folded-inference conv fwd: the kernel body, grid and PIPE / SWZ choices of
// mfma_conv2d_fwd with the wide epilogue,
//   out = bf16( [relu]( acc + bias[co] [+ float(res)] ) ),
// fp32 adds in that order and one rounding.  res has out's shape and layout
// (ignored unless has_res).  The 16-byte epilogue accesses need
// Cout % 8 == 0 and 16-byte aligned out / res.
void mfma_conv2d_fwd_fused(Tensor x, Tensor wgt, Tensor bias, Tensor res,
                           Tensor out, int64_t N, int64_t H, int64_t W,
                           int64_t Cin, int64_t P, int64_t Q, int64_t Cout,
                           int64_t KH, int64_t KW, int64_t stride, int64_t pad,
                           bool relu, bool has_res) {
  const char* who = "mfma_conv2d_fwd_fused";
  const ConvGeom g{N, H, W, Cin, P, Q, Cout, KH, KW, stride, pad};
  const dwtmm::ConvParams cp = conv_params(who, g, false);
  check_operands(who, {{"x", x, at::kBFloat16, N * H * W * Cin},
                       {"wgt", wgt, at::kBFloat16, Cout * cp.K},
                       {"bias", bias, at::kFloat, Cout},
                       {"out", out, at::kBFloat16, cp.M * Cout}});
  if (has_res) check_operands(who, {{"res", res, at::kBFloat16, cp.M * Cout}});
  TORCH_CHECK(Cout % 8 == 0, who, ": Cout % 8");
  TORCH_CHECK(P == (H + 2 * pad - KH) / stride + 1 &&
              Q == (W + 2 * pad - KW) / stride + 1, who, ": output extent");
  TORCH_CHECK(aligned16(out) && (!has_res || aligned16(res)), who,
              ": out / res alignment");
  const TilePlan tp = tile_plan(who, cp, g.unit(), Cin);
  auto go = [&](auto modec, auto reluc, auto resc, auto pipec, auto swzc) {
    hipLaunchKernelGGL(
        (dwtmm::conv_fused_fwd_kernel<decltype(modec)::value,
                                      decltype(reluc)::value,
                                      decltype(resc)::value,
                                      decltype(pipec)::value,
                                      decltype(swzc)::value>),
        dim3(tp.mtiles * tp.ntiles), dim3(dwtmm::THREADS), 0, dwtmm_stream(),
        (const c10::BFloat16*)x.data_ptr(), (const c10::BFloat16*)wgt.data_ptr(),
        bias.data_ptr<float>(),
        has_res ? (const c10::BFloat16*)res.data_ptr() : nullptr,
        (c10::BFloat16*)out.data_ptr(), cp, tp.mtiles, tp.ntiles);
  };
  if (tp.gemm_fast)
    static_dispatch(
        [&](auto r, auto s, auto p, auto z) { go(ADense{}, r, s, p, z); }, relu,
        has_res, tp.pipe, tp.swz);
  else
    static_dispatch([&](auto r, auto s) { go(AConv{}, r, s, kOff, kOff); },
                    relu, has_res);
}


// 1x1 stride-1 conv forward + the next norm site's raw statistics.
// x: raw NHWC storage of M = numel/Cin positions; wgt (Cout, Cin) storage;
// out raw NHWC (M, Cout); acc fp32, ZEROED by the caller, laid out as the
// finalize kernels read it (see conv1x1_stats_kernel).  kind: 0 = BN,
// 1 = whitening (g must be 4).  max_workgroups: 0 = one resident wave of
// workgroups for this device; tests pass 1 or 2 to force long runs.
void conv1x1_stats(Tensor x, Tensor wgt, Tensor out, Tensor acc, int64_t kind,
                   int64_t g, int64_t parts, int64_t max_workgroups) {
  const char* who = "conv1x1_stats";
  TORCH_CHECK(wgt.dim() >= 2 && wgt.size(0) > 0 && wgt.numel() > 0 &&
              acc.is_contiguous(), who, ": wgt / acc layout");
  const int64_t Cout = wgt.size(0);
  const int64_t Cin = wgt.numel() / Cout;
  TORCH_CHECK(Cin % 8 == 0 && Cout % 8 == 0, who, ": C % 8");
  TORCH_CHECK(x.numel() % Cin == 0, who, ": x size");
  const int64_t M = x.numel() / Cin;
  TORCH_CHECK(parts >= 1 && M % parts == 0 && (M / parts) % dwtmm::BM == 0,
              who, ": rows per branch must be a multiple of ", dwtmm::BM);
  TORCH_CHECK(kind == dwtmm::STATS_BN || (kind == dwtmm::STATS_WHITEN4 && g == 4),
              who, ": BN or whitening with g = 4 only");
  check_operands(who, {{"x", x, at::kBFloat16, M * Cin},
                       {"wgt", wgt, at::kBFloat16, Cout * Cin},
                       {"out", out, at::kBFloat16, M * Cout},
                       {"acc", acc, at::kFloat,
                        kind == dwtmm::STATS_BN ? parts * 2 * Cout
                                                : parts * (Cout / 4) * 20}});
  const dwtmm::ConvParams cp = gemm_params(who, M, Cin, Cout);
  const TilePlan tp = tile_plan(who, cp, true, Cin);
  const bool glds = dense_glds_ok(x, wgt, out, cp);
  int64_t maxwg = max_workgroups;
  if (maxwg <= 0) {
    // queried once: the CU count of whichever device is current on the
    // first call serves every device (the supported boxes are homogeneous)
    static const int cus =
        at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
    maxwg = (int64_t)cus * ((tp.pipe || glds) ? 2 : 3);
  }
  const int nlanes = (int)std::min<int64_t>(maxwg, tp.ntiles);
  const int runs = (int)std::max<int64_t>(
      1, std::min<int64_t>(maxwg / nlanes, tp.mtiles));
  // both kernels take the same arguments
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(
        kernel, dim3(nlanes * runs), dim3(dwtmm::THREADS), 0, dwtmm_stream(),
        (const c10::BFloat16*)x.data_ptr(), (const c10::BFloat16*)wgt.data_ptr(),
        (c10::BFloat16*)out.data_ptr(), acc.data_ptr<float>(), cp, tp.mtiles,
        tp.ntiles, (int)(M / parts / dwtmm::BM), nlanes, runs);
  };
  const OneOf<dwtmm::STATS_BN, dwtmm::STATS_WHITEN4> kinds{kind};
  if (glds) {
    static_dispatch([&](auto k) {
      launch(dwtmm::conv1x1_stats_glds_kernel<decltype(k)::value>);
    }, kinds);
    ++g_dense_glds_launches;
  } else {
    static_dispatch([&](auto p, auto k) {
      launch(dwtmm::conv1x1_stats_kernel<decltype(p)::value, decltype(k)::value>);
    }, tp.pipe, kinds);
  }
}


// dgrad: dx (N,H,W,Cin) = implicit-GEMM over dy (N,P,Q,Cdy) with
// wd (Cin, KH*KW*Cdy) = weight permuted to [ci][r][s][co] (host side).
void mfma_conv2d_dgrad(Tensor dy, Tensor wd, Tensor dx, int64_t N, int64_t H,
                       int64_t W, int64_t Cin, int64_t P, int64_t Q,
                       int64_t Cdy, int64_t KH, int64_t KW, int64_t stride,
                       int64_t pad) {
  const char* who = "mfma_conv2d_dgrad";
  const ConvGeom g{N, H, W, Cin, P, Q, Cdy, KH, KW, stride, pad};
  const dwtmm::ConvParams cp = conv_params(who, g, true);
  check_operands(who, {{"dy", dy, at::kBFloat16, N * P * Q * Cdy},
                       {"wd", wd, at::kBFloat16, Cin * cp.K},
                       {"dx", dx, at::kBFloat16, cp.M * Cin}});
  // 1x1/stride-1 dgrad IS the dense GEMM dy @ w^T — tile_plan puts it on the
  // pipelined/swizzled dense path instead of the per-chunk gather decode
  const TilePlan tp = tile_plan(who, cp, g.unit(), Cdy);
  if (tp.gemm_fast || stride == 1 || cp.cShift < 0 || Cdy < 8) {
    launch_conv_gemm(dwtmm::A_DGRAD, dy, wd, nullptr, dx, cp, tp, false);
    return;
  }
  // class decomposition: one launch per (h%stride, w%stride) residue
  for (int ch = 0; ch < stride; ++ch) {
    for (int cw = 0; cw < stride; ++cw) {
      dwtmm::DgradClsParams gp{};
      gp.H = H; gp.W = W; gp.Cin = Cin; gp.P = P; gp.Q = Q;
      gp.Cdy = Cdy; gp.Kfull = cp.K;
      gp.ch = ch; gp.cw = cw; gp.stride = stride;
      gp.Hc = (int)((H - ch + stride - 1) / stride);
      gp.Wc = (int)((W - cw + stride - 1) / stride);
      gp.M = (int64_t)N * gp.Hc * gp.Wc;
      gp.cShift = cp.cShift;
      int rl[16], sl[16], nr = 0, ns = 0;
      for (int r = 0; r < KH; ++r)
        if ((ch + pad - r) % stride == 0 && nr < 4) rl[nr++] = r;
      for (int s = 0; s < KW; ++s)
        if ((cw + pad - s) % stride == 0 && ns < 4) sl[ns++] = s;
      int ntaps = 0;
      for (int a = 0; a < nr && ntaps < 16; ++a)
        for (int b = 0; b < ns && ntaps < 16; ++b) {
          gp.dp[ntaps] = (int)((ch + pad - rl[a]) / stride);
          gp.dq[ntaps] = (int)((cw + pad - sl[b]) / stride);
          gp.rsIdx[ntaps] = rl[a] * KW + sl[b];
          ++ntaps;
        }
      gp.K = ntaps * Cdy;
      if (ntaps == 0 || gp.M == 0) continue;
      // gp.M <= cp.M: the class grid fits wherever the plan's does
      const int cm = (int)((gp.M + dwtmm::BM - 1) / dwtmm::BM);
      hipLaunchKernelGGL(dwtmm::dgrad_cls_kernel, dim3(cm * tp.ntiles),
                         dim3(dwtmm::THREADS), 0, dwtmm_stream(),
                         (const c10::BFloat16*)dy.data_ptr(),
                         (const c10::BFloat16*)wd.data_ptr(),
                         (c10::BFloat16*)dx.data_ptr(), gp, cm, tp.ntiles);
    }
  }
}


// wgrad v2 (split-K): dy (N,P,Q,Cout) raw NHWC, x (N,H,W,Cin) raw NHWC,
// ws fp32 zero-initialized [Cout, KH*KW*Cin], dw bf16 channels_last weight
// storage (same [co][r][s][ci] flat layout as ws).  Cout % 8 == 0 (the dy
// tile loads 16 bytes at a time).
// ConvParams reuse here: cp.N = Cout (dy channel stride), cp.Cout =
// KH*KW*Cin (dw columns), cp.M = real NPQ.
void mfma_conv2d_wgrad(Tensor dy, Tensor x, Tensor dw, Tensor ws, int64_t N,
                       int64_t H, int64_t W, int64_t Cin, int64_t P,
                       int64_t Q, int64_t Cout, int64_t KH, int64_t KW,
                       int64_t stride, int64_t pad) {
  const char* who = "mfma_conv2d_wgrad";
  const ConvGeom g{N, H, W, Cin, P, Q, Cout, KH, KW, stride, pad};
  dwtmm::ConvParams cp = conv_params(who, g, false);
  const int64_t n = (int64_t)Cout * cp.K;      // elements of dw
  check_operands(who, {{"dy", dy, at::kBFloat16, cp.M * Cout},
                       {"x", x, at::kBFloat16, N * H * W * Cin},
                       {"dw", dw, at::kBFloat16, n},
                       {"ws", ws, at::kFloat, n}});
  TORCH_CHECK(Cout % 8 == 0, who, ": Cout % 8");
  cp.N = Cout;
  cp.Cout = cp.K;
  // 128 tile when both dims fill it (4x less cross-tile operand traffic);
  // 64 tile otherwise (stem/l1 shapes would waste half the MFMA work)
  const int WT = (Cout >= 128 && cp.Cout >= 128) ? 128 : 64;
  const int mtiles = (int)((Cout + WT - 1) / WT);
  const int ntiles = (cp.Cout + WT - 1) / WT;
  TORCH_CHECK((int64_t)mtiles * ntiles < (int64_t)1 << 31 &&
              (n + 255) / 256 < (int64_t)1 << 31, who,
              ": grid does not fit 32 bits");
  // split K so the grid lands at >=2048 workgroups (256 CUs, several waves
  // deep), k-slabs rounded to whole BK tiles
  int64_t splitk = std::max<int64_t>(1, 2048 / (mtiles * ntiles));
  const int64_t kt = (cp.M + dwtmm::WBK - 1) / dwtmm::WBK;  // total k-tiles
  splitk = std::min<int64_t>(splitk, kt);
  const int64_t klen = ((kt + splitk - 1) / splitk) * dwtmm::WBK;
  static_dispatch([&](auto ac, auto wtc) {
    hipLaunchKernelGGL(
        (dwtmm::wgrad_splitk_kernel<decltype(ac)::value, decltype(wtc)::value>),
        dim3(mtiles * ntiles * splitk), dim3(256), 0, dwtmm_stream(),
        (const c10::BFloat16*)dy.data_ptr(), (const c10::BFloat16*)x.data_ptr(),
        ws.data_ptr<float>(), cp, mtiles, ntiles, (int)splitk, klen);
  }, Cin % 64 == 0, OneOf<64, 128>{WT});
  hipLaunchKernelGGL(dwtmm::f32_to_bf16_kernel, dim3((n + 255) / 256),
                     dim3(256), 0, dwtmm_stream(), ws.data_ptr<float>(),
                     (c10::BFloat16*)dw.data_ptr(), n);
}
