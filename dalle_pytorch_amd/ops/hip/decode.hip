// Single-token decode family: fused sampler, the sk2 weights-streaming GEMM,
// the residual + LayerNorm + shift prelude, key-split decode attention and
// the ring-buffer token shift.

#include "hip_host.h"

// ---------------------------------------------------------------------------
// Fused top-k + gumbel sampling for the decode loop (reference
// dalle_pytorch.py:53-69 semantics): one kernel replaces the ~12-kernel
// torch chain (mbtopk x4, scatter, full_like, log/neg/div/argmax...),
// which cost ~90 us of a ~1.3 ms decode step. Per row: stage logits in
// LDS, bisect the k-th-largest threshold (float bisection on the staged
// row — ties at the threshold are kept, which only differs from topk's
// index tie-break in the degenerate equal-logit case), then
// argmax(logit/temperature + gumbel(u)) over the kept set.
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256)
void sample_topk_gumbel_kernel(
    const float* __restrict__ logits,   // [rows, V], V <= 8192
    const float* __restrict__ noise,    // [rows, V] uniform(0,1)
    long* __restrict__ out,             // [rows] (doubles as the next feed)
    long* __restrict__ seq,             // [rows, S] generated-sequence buffer
    const long* __restrict__ seq_ptr,   // [1] write position, or null
    int S, int V, int k, float inv_temp) {
  // row cached in REGISTERS (32 values/thread @ V=8192): the LDS-staged
  // form spent ~42 us in bisection LDS sweeps; this runs the 24 bisection
  // rounds over registers with one tiny cross-wave reduce each
  __shared__ float red[8];
  __shared__ int redi[4];
  const int row = blockIdx.x;
  const int tid = threadIdx.x;
  const float* lr = logits + (long)row * V;

  // FIXED 32-slot register cache (dynamic trip counts spill to scratch);
  // out-of-range slots hold -inf and drop out of every reduction
  float v[32];
  #pragma unroll
  for (int j = 0; j < 32; ++j) {
    const int i = tid + j * 256;
    v[j] = i < V ? lr[i] : -INFINITY;
  }

  float mx = -INFINITY, mn = INFINITY;
  #pragma unroll
  for (int j = 0; j < 32; ++j) {
    mx = fmaxf(mx, v[j]);
    if (v[j] != -INFINITY) mn = fminf(mn, v[j]);
  }
  #pragma unroll
  for (int sft = 32; sft > 0; sft >>= 1) {
    mx = fmaxf(mx, __shfl_xor(mx, sft));
    mn = fminf(mn, __shfl_xor(mn, sft));
  }
  if ((tid & 63) == 0) { red[tid >> 6] = mx; red[4 + (tid >> 6)] = mn; }
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  mn = fminf(fminf(red[4], red[5]), fminf(red[6], red[7]));

  // bisect tau such that count(x > tau) < k <= count(x >= tau)
  float lo = mn, hi = mx;
  for (int it = 0; it < 24 && lo < hi; ++it) {
    const float mid = 0.5f * (lo + hi);
    int cnt = 0;
    #pragma unroll
    for (int j = 0; j < 32; ++j) cnt += v[j] > mid;
    #pragma unroll
    for (int sft = 32; sft > 0; sft >>= 1) cnt += __shfl_xor(cnt, sft);
    if ((tid & 63) == 0) redi[tid >> 6] = cnt;
    __syncthreads();
    cnt = redi[0] + redi[1] + redi[2] + redi[3];
    if (cnt >= k) lo = mid; else hi = mid;
    __syncthreads();
  }
  const float tau = lo;   // keep x >= tau (>= k elements incl. ties)

  // argmax over kept of logit/temp + gumbel(noise)
  const float* ur = noise + (long)row * V;
  float best = -INFINITY;
  int besti = 0;
  #pragma unroll 8
  for (int j = 0; j < 32; ++j) {
    const float x = v[j];
    if (x < tau) continue;
    const int i = tid + j * 256;
    float u = fmaxf(ur[i], 1e-20f);
    float g = -__logf(fmaxf(-__logf(u), 1e-20f));
    const float sc = x * inv_temp + g;
    if (sc > best) { best = sc; besti = i; }
  }
  #pragma unroll
  for (int sft = 32; sft > 0; sft >>= 1) {
    const float ob = __shfl_xor(best, sft);
    const int oi = __shfl_xor(besti, sft);
    if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
  }
  __syncthreads();
  if ((tid & 63) == 0) {
    red[tid >> 6] = best;
    redi[tid >> 6] = besti;
  }
  __syncthreads();
  if (tid == 0) {
    best = red[0]; besti = redi[0];
    #pragma unroll
    for (int w = 1; w < 4; ++w) {
      if (red[w] > best || (red[w] == best && redi[w] < besti)) {
        best = red[w];
        besti = redi[w];
      }
    }
    out[row] = besti;
    // fold the sequence-buffer write into the same dispatch (replaces the
    // eager index_copy_ kernel + its index plumbing in the decode graph)
    if (seq != nullptr) seq[(long)row * S + *seq_ptr] = besti;
  }
}

// ---------------------------------------------------------------------------
// sk2: second-generation decode GEMM, out[M, N] = x[M, K] @ W[N, K]^T (+bias),
// M in {16, 32, 64, 128}. One kernel, fused epilogue, no trailing cast pass.
//
// The token-decode projections are tiny-M GEMMs against multi-MB weights —
// pure weight-streaming problems that hipBLASLt executes at 12-14 us inside
// the decode graph (measured profiles/rocprof_generate_r2b.txt: 51% of the
// whole token step) against a ~1-3 us weight-read roofline. Design:
//   * W is pre-packed ONCE on the host (decode weights are static) into MFMA
//     A-fragment order [N/16][K/32][lane][8], so each wave streams ONE fully
//     contiguous region of HBM with dwordx4 loads — no strided access, no LDS
//     staging, no shared-memory bank concerns.
//   * One workgroup per 16-column tile of W; its 4 waves split K four ways
//     (grid = N/16 >= 64 blocks even for the square out-proj, vs the 48-tile
//     starved hipBLASLt MT64x64 launch). Partials meet in LDS; the epilogue
//     (bias add + bf16 cast, the GEGLU gate product, or an fp32 store for the
//     sampler head) runs in the same kernel.
//   * x ([M,K] <= 256 KB) stays L2-resident and is read directly as MFMA
//     B-fragments; the 4x re-read across waves is free next to W traffic.
//   * Loads are software-pipelined DEPTH chunks ahead with compile-time ring
//     indices (a dynamic ring index spills the staging array to scratch —
//     the sample_topk lesson).
// MODE 0: bias epilogue. MODE 1: GEGLU pair — this block also streams the
// gate tile at column nt*16 + N/2 and writes value*gelu(gate) (out width
// N/2), replacing the separate geglu kernel dispatch. MODE 2: fp32 out+bias
// (the image-vocab head feeding the fp32 sampler).
// ---------------------------------------------------------------------------

// F8 = true streams e4m3 weights (HALF the bytes of the weight-bound
// stream; the non-scaled 16x16x32_fp8_fp8 MFMA runs at the bf16 rate, which
// is irrelevant here) and converts the L2-resident bf16 activations to fp8
// in-register (the kernel is latency-bound with idle VALU). One per-tensor
// weight scale is folded into the epilogue; activations ride unscaled
// (post-LN magnitudes sit far inside e4m3's +-448 range; clamped anyway).
// Opt-in quality trade (DALLE_AMD_FP8_DECODE=1) — the bf16 path is default.
template <int MT, int MODE, int KS = 4, bool F8 = false>
__global__ __launch_bounds__(KS * 64, 2)
void sk2_kernel(const short* __restrict__ x,     // [MT*16, K] bf16
                const short* __restrict__ wp,    // packed [N/16][K/32][64][8]
                const float* __restrict__ bias,  // [N] fp32 or null
                void* __restrict__ out,          // [MT*16, NO]
                int N, int K, float wscale = 1.f) {
  constexpr int NW = (MODE == 1) ? 2 : 1;        // weight streams per block
  // ring depth bounds the per-wave outstanding loads (the compiler drains
  // vmcnt(0) once per ring cycle, so bytes-in-flight = DEPTH * frags * 16 B);
  // deeper is faster until VGPR staging (DEPTH * (NW + MT) * 4 regs) costs
  // occupancy. KCW % DEPTH == 0 must hold (K % 512 == 0 gives KCW in 8/16/32).
  constexpr int DEPTH = (NW == 2 && MT >= 4) ? 2
                        : (MT >= 8 ? 4 : 8);
  const int nt = blockIdx.x;
  const int wave = threadIdx.x >> 6;             // = this wave's k-split
  const int lane = threadIdx.x & 63;
  const int lq = lane & 15;
  const int kg = lane >> 4;
  const int KC = K >> 5;                         // 32-wide k-chunks total
  const int KCW = KC / KS;                       // chunks per wave
  const long tile_elems = (long)KC * 512;        // shorts per packed n-tile

  // fp8 packs are bytes at the same [nt][kc][lane][8] indexing
  const char* wraw = reinterpret_cast<const char*>(wp);
  const long esz = F8 ? 1 : 2;
  const char* wb0 = wraw + ((long)nt * tile_elems
                        + ((long)wave * KCW) * 512 + lane * 8) * esz;
  const char* wb1 = (MODE == 1)
      ? wraw + (((long)nt + (N >> 5)) * tile_elems
           + ((long)wave * KCW) * 512 + lane * 8) * esz
      : nullptr;
  const short* xb = x + (long)lq * K + kg * 8 + (long)wave * KCW * 32;

  f32x4 acc[NW][MT];
  #pragma unroll
  for (int s = 0; s < NW; ++s)
    #pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[s][mt] = f32x4{0, 0, 0, 0};

  bf16x8 wrg[DEPTH][NW];
  bf16x8 xrg[DEPTH][MT];

  const long wstep = F8 ? 512 : 1024;   // bytes per (lane-sliced) chunk
  auto load_w = [&](const char* base, long idx) -> bf16x8 {
    if (F8) {   // 8 e4m3 bytes in the low half of the frag registers
      const int2 b8 = *reinterpret_cast<const int2*>(base + idx * wstep);
      bf16x8 f{};
      *reinterpret_cast<int2*>(&f) = b8;
      return f;
    }
    return *reinterpret_cast<const bf16x8*>(base + idx * wstep);
  };
  // bf16 -> e4m3 in-register: 8 clamps + 4 pack-converts per fragment
  auto to_fp8 = [&](bf16x8 v) -> long {
    const short* s = reinterpret_cast<const short*>(&v);
    unsigned lo = 0, hi = 0;
    #pragma unroll
    for (int p2 = 0; p2 < 2; ++p2) {
      const float a = fminf(fmaxf(bf2f(s[4 * p2]), -448.f), 448.f);
      const float b = fminf(fmaxf(bf2f(s[4 * p2 + 1]), -448.f), 448.f);
      const float c = fminf(fmaxf(bf2f(s[4 * p2 + 2]), -448.f), 448.f);
      const float d = fminf(fmaxf(bf2f(s[4 * p2 + 3]), -448.f), 448.f);
      unsigned& w32 = p2 ? hi : lo;
      w32 = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, w32, false);
      w32 = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w32, true);
    }
    return ((long)(unsigned long)hi << 32) | lo;
  };
  auto mfma_any = [&](bf16x8 wf, bf16x8 xf, f32x4 c) -> f32x4 {
    if (F8) {
      const long wa = *reinterpret_cast<const long*>(&wf);
      return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(wa, to_fp8(xf),
                                                        c, 0, 0, 0);
    }
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf, c, 0, 0, 0);
  };

  // prologue: fill the ring (KCW >= DEPTH, host-enforced via K % 1024 == 0)
  #pragma unroll
  for (int p = 0; p < DEPTH; ++p) {
    wrg[p][0] = load_w(wb0, p);
    if (MODE == 1)
      wrg[p][NW - 1] = load_w(wb1, p);
    #pragma unroll
    for (int mt = 0; mt < MT; ++mt)
      xrg[p][mt] = *reinterpret_cast<const bf16x8*>(xb + (long)mt * 16 * K
                                                       + (long)p * 32);
  }

  for (int base = 0; base < KCW; base += DEPTH) {
    #pragma unroll
    for (int p = 0; p < DEPTH; ++p) {
      __builtin_amdgcn_s_setprio(1);
      #pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        acc[0][mt] = mfma_any(wrg[p][0], xrg[p][mt], acc[0][mt]);
        if (MODE == 1)
          acc[NW - 1][mt] = mfma_any(wrg[p][NW - 1], xrg[p][mt],
                                     acc[NW - 1][mt]);
      }
      __builtin_amdgcn_s_setprio(0);
      const int nx = base + DEPTH + p;
      if (nx < KCW) {
        wrg[p][0] = load_w(wb0, nx);
        if (MODE == 1)
          wrg[p][NW - 1] = load_w(wb1, nx);
        #pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          xrg[p][mt] = *reinterpret_cast<const bf16x8*>(
              xb + (long)mt * 16 * K + (long)nx * 32);
      }
    }
  }

  // k-split reduce through LDS. Layout [wave][s][mt][n][m]; MFMA C frag:
  // m (x row) = lane&15, n (w row) = grp*4 + r.
  __shared__ float red[KS][NW][MT][16][16];
  #pragma unroll
  for (int s = 0; s < NW; ++s)
    #pragma unroll
    for (int mt = 0; mt < MT; ++mt)
      #pragma unroll
      for (int r = 0; r < 4; ++r)
        red[wave][s][mt][kg * 4 + r][lq] = acc[s][mt][r];
  __syncthreads();

  const int NO = (MODE == 1) ? (N >> 1) : N;
  for (int i = threadIdx.x; i < MT * 256; i += KS * 64) {
    const int mt = i >> 8, m = (i >> 4) & 15, n = i & 15;
    float v = 0.f, g = 0.f;
    #pragma unroll
    for (int s4 = 0; s4 < KS; ++s4) v += red[s4][0][mt][n][m];
    if (F8) v *= wscale;
    const long o = (long)(mt * 16 + m) * NO + nt * 16 + n;
    if (MODE == 1) {
      #pragma unroll
      for (int s4 = 0; s4 < KS; ++s4) g += red[s4][NW - 1][mt][n][m];
      if (F8) g *= wscale;
      if (bias != nullptr) {
        v += bias[nt * 16 + n];
        g += bias[(N >> 1) + nt * 16 + n];
      }
      reinterpret_cast<short*>(out)[o] = f2bf(v * gelu_f(g));
    } else {
      if (bias != nullptr) v += bias[nt * 16 + n];
      if (MODE == 2) reinterpret_cast<float*>(out)[o] = v;
      else           reinterpret_cast<short*>(out)[o] = f2bf(v);
    }
  }
}

// ---------------------------------------------------------------------------
// Decode prelude: residual-apply + LayerNorm + optional token-shift for one
// decode token, fused (the decode step is bound by a ~5 us per-kernel
// execution floor, so 3 tiny kernels -> 1 is a direct win x24 per step):
//   x_new = x (+ scale * y)            [the previous branch's residual]
//   z     = LN(x_new) * w + b
//   z     = token_shift(z) via the S-slot ring when ring != null
// One wave per batch row; dim = PER * 64.
// ---------------------------------------------------------------------------

template <int CPT>   // channels per thread = dim / 256
__global__ __launch_bounds__(256)
void dec_prelude_kernel(
    const short* __restrict__ x,      // [rows, dim]
    const short* __restrict__ y,      // [rows, dim] or null
    const float* __restrict__ scale,  // [dim] or null (with y)
    const float* __restrict__ w,      // LN gamma [dim]
    const float* __restrict__ bia,    // LN beta [dim]
    short* __restrict__ xn,           // [rows, dim] updated stream
    short* __restrict__ z,            // [rows, dim] LN(+shift) output
    short* __restrict__ ring,         // [rows, S, dim/2] or null
    const long* __restrict__ offset,  // [1]
    long rows, float eps, int S, int text_len) {
  constexpr int dim = CPT * 256;
  __shared__ float stat[8];
  const long row = blockIdx.x;
  const int tid = threadIdx.x;
  const int c0 = tid * CPT;
  const short* xr = x + row * (long)dim;
  const short* yr = y ? y + row * (long)dim : nullptr;

  float sum = 0.f, sq = 0.f;
  float vals[CPT];
  {
    // CPT is 2/4/8: load as that many shorts in one access
    #pragma unroll
    for (int e = 0; e < CPT; ++e) {
      float f = bf2f(xr[c0 + e]);
      if (yr) f += scale[c0 + e] * bf2f(yr[c0 + e]);
      vals[e] = f;
      sum += f;
      sq += f * f;
    }
    if (yr) {
      short upd[CPT];
      #pragma unroll
      for (int e = 0; e < CPT; ++e) upd[e] = f2bf(vals[e]);
      #pragma unroll
      for (int e = 0; e < CPT; ++e) xn[row * (long)dim + c0 + e] = upd[e];
    }
  }
  #pragma unroll
  for (int sft = 32; sft > 0; sft >>= 1) {
    sum += __shfl_xor(sum, sft);
    sq += __shfl_xor(sq, sft);
  }
  if ((tid & 63) == 0) {
    stat[tid >> 6] = sum;
    stat[4 + (tid >> 6)] = sq;
  }
  __syncthreads();
  sum = stat[0] + stat[1] + stat[2] + stat[3];
  sq = stat[4] + stat[5] + stat[6] + stat[7];
  const float mu = sum / dim;
  const float rstd = __frsqrt_rn(sq / dim - mu * mu + eps);

  constexpr int half = dim / 2, quarter = dim / 4;
  long pos = 0, prev = 0;
  bool row_start = false;
  if (ring != nullptr) {
    const long g0 = *offset - text_len;
    const long g = g0 < 0 ? 0 : g0;
    pos = g % S;
    prev = ((g - 1) % S + S) % S;
    row_start = (g % S) == 0;
  }
  short* rg = ring ? ring + (row * S) * (long)half : nullptr;
  short* zr = z + row * (long)dim;
  short out_c[CPT], ln_c[CPT];
  #pragma unroll
  for (int e = 0; e < CPT; ++e) {
    const int d = c0 + e;
    const short lnv = f2bf((vals[e] - mu) * rstd * w[d] + bia[d]);
    ln_c[e] = lnv;
    short o = lnv;
    if (ring != nullptr) {
      if (d < quarter) {
        o = rg[pos * half + d];
      } else if (d < half) {
        o = row_start ? (short)0 : rg[prev * half + d];
      }
    }
    out_c[e] = o;
  }
  if (ring != nullptr) {
    // write the ring slot AFTER its reads (same thread owns both)
    #pragma unroll
    for (int e = 0; e < CPT; ++e) {
      const int d = c0 + e;
      if (d < half) rg[pos * half + d] = ln_c[e];
    }
  }
  #pragma unroll
  for (int e = 0; e < CPT; ++e) zr[c0 + e] = out_c[e];
}

// ---------------------------------------------------------------------------
// Fused single-token decode attention, key-split ("flash decoding"; guide
// App. B "attention decode").
//
// The single-block-per-(b,head) form measured 144 us/dispatch at N=1281 —
// only b*h=1024 workgroups, each streaming its whole K/V slice through one
// CU, fully latency-bound (51.5% of generation GPU time, see
// profiles/decode_kernel_stats). Split the key range over KS extra grid
// blocks instead: each block softmaxes its chunk locally (lane-per-key
// dots on 16-byte K chunks — no shuffle reduces) and writes (m, l,
// acc[64]) partials; a tiny combine kernel merges the KS partials with the
// standard flash rescaling. b*h*KS blocks fill the chip and every K/V row
// is still read exactly once.
//
// Two dispatches rather than one kernel with an atomic-counter tail: the
// 8 XCDs have non-coherent L2s, so cross-block partial visibility would
// need device-scope fences on the hot path; the kernel boundary gives the
// same guarantee for one extra ~3 us launch.
// ---------------------------------------------------------------------------

constexpr int DEC_MAXN = 4096;
constexpr int DEC_CHUNK_MAX = 2048;   // chunk <= N/KS aligned, KS >= 2
constexpr int DEC_LMAX = 5376;        // one-pass kernel: live-list slots per block

// This token's q/k/v element d of (batch bi, head) out of the fused
// projection qkv [b, 3*h*64], rotary applied at position off (q unscaled).
DEVFN void dec_token_qkv(const short* qkv, const float* cosv,
                         const float* sinv,
                         long off, int bi, int head, int h, int rot, int d,
                         float* q_out, float* k_out, float* v_out) {
  const long base = (long)bi * 3 * h * 64 + (long)head * 64 + d;
  float qv = bf2f(qkv[base]);
  float kv = bf2f(qkv[base + (long)h * 64]);
  float vv = bf2f(qkv[base + 2L * h * 64]);
  if (d < rot && cosv != nullptr) {
    const int prt = d ^ 1;                        // pair partner
    const float cs = cosv[off * rot + d];
    const float sn = sinv[off * rot + d];
    const float sgn = (d & 1) ? 1.f : -1.f;       // even: -x_{d+1}, odd: +x_{d-1}
    const long pbase = (long)bi * 3 * h * 64 + (long)head * 64 + prt;
    qv = qv * cs + sgn * bf2f(qkv[pbase]) * sn;
    kv = kv * cs + sgn * bf2f(qkv[pbase + (long)h * 64]) * sn;
    vv = vv * cs + sgn * bf2f(qkv[pbase + 2L * h * 64]) * sn;
  }
  *q_out = qv;
  *k_out = kv;
  *v_out = vv;
}

__global__ __launch_bounds__(256)
void fa_decode_part_kernel(
    const short* __restrict__ qkv,    // [b, 3*h*64] (this token's projection)
    short* __restrict__ kc,           // [b, h, N, 64]
    short* __restrict__ vc,           // [b, h, N, 64]
    const float* __restrict__ cosv,   // [Ncos, rot] or null
    const float* __restrict__ sinv,
    const long* __restrict__ offset,  // [1] current position
    const bool* __restrict__ pattern, // [N, N] or null; row = *offset
    float* __restrict__ scratch,      // [b, h, KS, 66] = m, l, acc[64]
    int b, int h, int N, int rot, float scale, int KS, int chunk) {

  __shared__ float qs[64], ksn[64], vsn[64];
  __shared__ float Pl[DEC_CHUNK_MAX];
  __shared__ float red[4 * 64];
  __shared__ float stat[8];

  const int head = blockIdx.x, bi = blockIdx.y, z = blockIdx.z;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const long off = *offset;

  // ---- rope for this token (threads 0..63, d = tid); every block computes
  // it (cheap) so no block ever reads the fresh cache row another block
  // wrote — block z==0 alone persists it to the caches.
  if (tid < 64) {
    const int d = tid;
    float qv, kv, vv;
    dec_token_qkv(qkv, cosv, sinv, off, bi, head, h, rot, d, &qv, &kv, &vv);
    if (z == 0) {
      const long cbase = (((long)bi * h + head) * N + off) * 64 + d;
      kc[cbase] = f2bf(kv);
      vc[cbase] = f2bf(vv);
    }
    qs[d] = qv * (scale * 1.44269504088896f);
    ksn[d] = kv;
    vsn[d] = vv;
  }
  __syncthreads();

  // ---- dots over this block's key chunk: one LANE per key, K row read as
  // 8x int4v (the full 128-byte row is consumed across the 8 chunks)
  const long s0 = (long)z * chunk;
  const bool* prow = pattern ? pattern + off * N : nullptr;
  const short* krow0 = kc + ((long)bi * h + head) * N * 64;
  for (int base = wave * 64; base < chunk; base += 256) {
    const long key = s0 + base + lane;
    float dot = NEG_INF;
    if (key <= off && (prow == nullptr || prow[key])) {
      float p = 0.f;
      if (key == off) {
        #pragma unroll
        for (int d = 0; d < 64; ++d) p += qs[d] * ksn[d];
      } else {
        const short* krow = krow0 + key * 64;
        #pragma unroll
        for (int c = 0; c < 8; ++c) {
          int4v kk = *reinterpret_cast<const int4v*>(krow + c * 8);
          const short* ks = reinterpret_cast<const short*>(&kk);
          #pragma unroll
          for (int e = 0; e < 8; ++e) p += qs[c * 8 + e] * bf2f(ks[e]);
        }
      }
      dot = p;
    }
    Pl[base + lane] = dot;
  }
  __syncthreads();

  // ---- chunk-local softmax stats
  float m = NEG_INF;
  for (int i = tid; i < chunk; i += 256) m = fmaxf(m, Pl[i]);
  #pragma unroll
  for (int s = 32; s > 0; s >>= 1) m = fmaxf(m, __shfl_xor(m, s));
  if (lane == 0) stat[wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(stat[0], stat[1]), fmaxf(stat[2], stat[3]));

  float lsum = 0.f;
  for (int i = tid; i < chunk; i += 256) {
    const float p = (Pl[i] == NEG_INF || m == NEG_INF)
        ? 0.f : fexp2(Pl[i] - m);
    Pl[i] = p;
    lsum += p;
  }
  #pragma unroll
  for (int s = 32; s > 0; s >>= 1) lsum += __shfl_xor(lsum, s);
  if (lane == 0) stat[4 + wave] = lsum;
  __syncthreads();
  const float l_loc = stat[4] + stat[5] + stat[6] + stat[7];

  // ---- P*V over the chunk: lane = d, wave-strided keys, coalesced V rows
  const short* vrow0 = vc + ((long)bi * h + head) * N * 64;
  float acc = 0.f;
  for (int i = wave; i < chunk; i += 4) {
    const float p = Pl[i];
    if (p != 0.f) {
      const long key = s0 + i;
      const float vv = (key == off) ? vsn[lane]
                                    : bf2f(vrow0[key * 64 + lane]);
      acc += p * vv;
    }
  }
  red[wave * 64 + lane] = acc;
  __syncthreads();
  if (wave == 0) {
    float* sl = scratch + (((long)bi * h + head) * KS + z) * 66;
    sl[2 + lane] = red[lane] + red[64 + lane] + red[128 + lane] +
        red[192 + lane];
    if (lane == 0) { sl[0] = m; sl[1] = l_loc; }
  }
}

// Live-list variant: the decoder precomputes, per attention layer and per
// offset row, the indices of the keys the pattern+causality actually allow
// (~288 of 1281 under the flagship axial patterns). Blocks iterate listed
// keys only — every K/V row loaded is a live one.
//
// FOUR heads per 256-thread block, one wave per head: at ~288 live keys a
// one-wave-per-(head, part) launch is dispatch-rate bound (5120 blocks ~
// 47.8 us/dispatch vs ~5 us of live traffic, profiled round 1) — packing 4
// heads per block cuts the block count 4x. Waves stay independent (private
// LDS slices, per-wave shuffle reductions); the single __syncthreads covers
// the q/k/v broadcast.
__global__ __launch_bounds__(256)
void fa_decode_part_list_kernel(
    const short* __restrict__ qkv,    // [b, 3*h*64]
    short* __restrict__ kc,           // [b, h, N, 64]
    short* __restrict__ vc,
    const float* __restrict__ cosv,
    const float* __restrict__ sinv,
    const long* __restrict__ offset,  // [1]
    const int* __restrict__ live,     // [N, Lmax] key indices per offset row
    const int* __restrict__ live_cnt, // [N]
    float* __restrict__ scratch,      // [b, h, KS, 66]
    int b, int h, int N, int rot, float scale, int KS, int chunk, int Lmax) {

  __shared__ float qs[4][64], ksn[4][64], vsn[4][64];
  __shared__ float Pl[4][64];
  __shared__ int   Ki[4][64];

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int head = blockIdx.x * 4 + wave;
  const int bi = blockIdx.y, z = blockIdx.z;
  const long off = *offset;
  const bool head_ok = head < h;

  if (head_ok) {
    const int d = lane;
    float qv, kv, vv;
    dec_token_qkv(qkv, cosv, sinv, off, bi, head, h, rot, d, &qv, &kv, &vv);
    if (z == 0) {
      const long cbase = (((long)bi * h + head) * N + off) * 64 + d;
      kc[cbase] = f2bf(kv);
      vc[cbase] = f2bf(vv);
    }
    qs[wave][d] = qv * (scale * 1.44269504088896f);
    ksn[wave][d] = kv;
    vsn[wave][d] = vv;
  }
  __syncthreads();
  if (!head_ok) return;

  const int cnt = live_cnt[off];
  const int j0 = z * 64;
  const int jn = min(64, cnt - j0);             // live entries in this part
  const int* lrow = live + off * (long)Lmax;
  const short* krow0 = kc + ((long)bi * h + head) * N * 64;

  // dots: one lane per listed key; the index load doubles as the mask
  float dot = NEG_INF;
  int key = -1;
  if (lane < jn) key = lrow[j0 + lane];
  if (key >= 0) {
    float p = 0.f;
    if (key == (int)off) {
      #pragma unroll
      for (int d = 0; d < 64; ++d) p += qs[wave][d] * ksn[wave][d];
    } else {
      const short* krow = krow0 + (long)key * 64;
      #pragma unroll
      for (int c = 0; c < 8; ++c) {
        int4v kk = *reinterpret_cast<const int4v*>(krow + c * 8);
        const short* ks = reinterpret_cast<const short*>(&kk);
        #pragma unroll
        for (int e = 0; e < 8; ++e) p += qs[wave][c * 8 + e] * bf2f(ks[e]);
      }
    }
    dot = p;
  }

  // wave-local softmax stats by shuffle
  float m = dot;
  #pragma unroll
  for (int s = 32; s > 0; s >>= 1) m = fmaxf(m, __shfl_xor(m, s));
  const float p = (dot == NEG_INF || m == NEG_INF) ? 0.f : fexp2(dot - m);
  float lsum = p;
  #pragma unroll
  for (int s = 32; s > 0; s >>= 1) lsum += __shfl_xor(lsum, s);

  Pl[wave][lane] = p;
  Ki[wave][lane] = key;
  // same-wave produce/consume: no cross-wave barrier needed

  // P*V: lane = d over this part's listed keys. 4 independent partial
  // accumulators keep 4 V-row loads in flight — the branchy serial form
  // was one 128 B line per ~HBM latency (49 us/dispatch profiled); every
  // listed key is live by construction so no zero-p branch is needed.
  const short* vrow0 = vc + ((long)bi * h + head) * N * 64;
  float a4[4] = {0.f, 0.f, 0.f, 0.f};
  int i = 0;
  for (; i + 4 <= jn; i += 4) {
    #pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int ki = Ki[wave][i + u];
      const float vv = (ki == (int)off) ? vsn[wave][lane]
                                        : bf2f(vrow0[(long)ki * 64 + lane]);
      a4[u] += Pl[wave][i + u] * vv;
    }
  }
  for (; i < jn; ++i) {
    const int ki = Ki[wave][i];
    const float vv = (ki == (int)off) ? vsn[wave][lane]
                                      : bf2f(vrow0[(long)ki * 64 + lane]);
    a4[0] += Pl[wave][i] * vv;
  }
  const float acc = (a4[0] + a4[1]) + (a4[2] + a4[3]);
  float* sl = scratch + (((long)bi * h + head) * KS + z) * 66;
  sl[2 + lane] = acc;
  if (lane == 0) { sl[0] = m; sl[1] = lsum; }
}

// One-pass decode attention over the live-key list: with the flagship axial
// patterns a head sees <=352 live keys, little enough that ONE wave handles
// the whole head (lane-parallel dots, shuffle softmax, unrolled PV with 4
// loads in flight) — no key-split scratch, no combine kernel, KS=1. Four
// heads per 256-thread block; grid (ceil(h/4), b).
__global__ __launch_bounds__(256)
void fa_decode_one_kernel(
    const short* __restrict__ qkv,    // [b, 3*h*64]
    short* __restrict__ kc,           // [b, h, N, 64]
    short* __restrict__ vc,
    const float* __restrict__ cosv,
    const float* __restrict__ sinv,
    const long* __restrict__ offset,  // [1]
    const int* __restrict__ live,     // [N, Lmax]
    const int* __restrict__ live_cnt, // [N]
    short* __restrict__ out,          // [b, h*64]
    int b, int h, int N, int rot, float scale, int Lmax) {

  __shared__ float qs[4][64], ksn[4][64], vsn[4][64];
  __shared__ float Pl[4][DEC_LMAX / 4];
  __shared__ int   Ki[4][DEC_LMAX / 4];

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int head = blockIdx.x * 4 + wave;
  const int bi = blockIdx.y;
  const long off = *offset;
  const bool head_ok = head < h;

  if (head_ok) {
    const int d = lane;
    float qv, kv, vv;
    dec_token_qkv(qkv, cosv, sinv, off, bi, head, h, rot, d, &qv, &kv, &vv);
    const long cbase = (((long)bi * h + head) * N + off) * 64 + d;
    kc[cbase] = f2bf(kv);
    vc[cbase] = f2bf(vv);
    qs[wave][d] = qv * (scale * 1.44269504088896f);
    ksn[wave][d] = kv;
    vsn[wave][d] = vv;
  }
  __syncthreads();
  if (!head_ok) return;

  const int jn = live_cnt[off];
  const int* lrow = live + off * (long)Lmax;
  const short* krow0 = kc + ((long)bi * h + head) * N * 64;

  // dots: lane-parallel over the listed keys, two rows per lane in flight
  float m_loc = NEG_INF;
  // branch-free: this block wrote its own heads' kc/vc rows (incl. the
  // current position) before the barrier, so key==off needs no special
  // case — and without the branch the loads pipeline instead of
  // serializing on vmcnt(0) (ISA-verified; was ~700 ns per key)
  auto dot_one = [&](int j) {
    const int key = lrow[j];
    const short* krow = krow0 + (long)key * 64;
    int4v kk[8];
    #pragma unroll
    for (int c = 0; c < 8; ++c)
      kk[c] = *reinterpret_cast<const int4v*>(krow + c * 8);
    float p = 0.f;
    #pragma unroll
    for (int c = 0; c < 8; ++c) {
      const short* ks = reinterpret_cast<const short*>(&kk[c]);
      #pragma unroll
      for (int e = 0; e < 8; ++e) p += qs[wave][c * 8 + e] * bf2f(ks[e]);
    }
    Pl[wave][j] = p;
    Ki[wave][j] = key;
    m_loc = fmaxf(m_loc, p);
  };
  int j = lane;
  for (; j + 128 < jn; j += 192) {
    dot_one(j);
    dot_one(j + 64);
    dot_one(j + 128);
  }
  for (; j < jn; j += 64) dot_one(j);
  #pragma unroll
  for (int s = 32; s > 0; s >>= 1) m_loc = fmaxf(m_loc, __shfl_xor(m_loc, s));

  float l_loc = 0.f;
  for (int j = lane; j < jn; j += 64) {
    const float p = fexp2(Pl[wave][j] - m_loc);
    Pl[wave][j] = p;
    l_loc += p;
  }
  #pragma unroll
  for (int s = 32; s > 0; s >>= 1) l_loc += __shfl_xor(l_loc, s);
  const float inv = l_loc > 0.f ? 1.f / l_loc : 0.f;

  // PV with a key-group split: lane = (kg 0..3) x (dd 0..15); each lane
  // covers d = 4*dd..4*dd+3 via one 8-byte V load and walks keys kg, kg+4,
  // ... — 4-way key parallelism x 4 loads in flight instead of one V row
  // per HBM latency.
  const short* vrow0 = vc + ((long)bi * h + head) * N * 64;
  const int kg = lane >> 4, dd = lane & 15;
  const int d0 = dd * 4;
  float a4[4][4];
  #pragma unroll
  for (int u = 0; u < 4; ++u)
    #pragma unroll
    for (int e = 0; e < 4; ++e) a4[u][e] = 0.f;
  auto pv_one = [&](int j, float* a) {
    const int ki = Ki[wave][j];
    const float pj = Pl[wave][j];
    const bf16x4 v4 = *reinterpret_cast<const bf16x4*>(
        vrow0 + (long)ki * 64 + d0);
    #pragma unroll
    for (int e = 0; e < 4; ++e) a[e] += pj * bf2f(v4[e]);
  };
  int i = kg;
  for (; i + 60 < jn; i += 64) {
    #pragma unroll
    for (int u = 0; u < 16; ++u) pv_one(i + 4 * u, a4[u & 3]);
  }
  for (; i + 12 < jn; i += 16) {
    #pragma unroll
    for (int u = 0; u < 4; ++u) pv_one(i + 4 * u, a4[u]);
  }
  for (; i < jn; i += 4) pv_one(i, a4[0]);
  #pragma unroll
  for (int e = 0; e < 4; ++e) {
    float s = (a4[0][e] + a4[1][e]) + (a4[2][e] + a4[3][e]);
    s += __shfl_xor(s, 16);       // fold the 4 key groups
    s += __shfl_xor(s, 32);
    if (kg == 0)
      out[(long)bi * h * 64 + head * 64 + d0 + e] = f2bf(s * inv);
  }
}

__global__ __launch_bounds__(256)
void fa_decode_combine_kernel(
    const float* __restrict__ scratch,  // [b, h, KS, 66]
    short* __restrict__ out,            // [b, h*64]
    int b, int h, int KS) {
  const int head = blockIdx.x * 4 + (threadIdx.x >> 6), bi = blockIdx.y;
  const int lane = threadIdx.x & 63;
  if (head >= h) return;
  const float* s0 = scratch + ((long)bi * h + head) * KS * 66;
  float m = NEG_INF;
  for (int z = 0; z < KS; ++z) m = fmaxf(m, s0[z * 66]);
  float den = 0.f, acc = 0.f;
  if (m != NEG_INF) {
    for (int z = 0; z < KS; ++z) {
      const float mz = s0[z * 66];
      if (mz == NEG_INF) continue;
      const float r = fexp2(mz - m);
      den += s0[z * 66 + 1] * r;
      acc += s0[z * 66 + 2 + lane] * r;
    }
  }
  out[(long)bi * h * 64 + (long)head * 64 + lane] =
      f2bf(den > 0.f ? acc / den : 0.f);
}

// ---------------------------------------------------------------------------
// Fused single-token token-shift (ring-buffer form): out token gets its
// first quarter from ring[g % S] (the grid row above), second quarter from
// ring[(g-1) % S] (left neighbor, zeroed at column 0), then the ring slot
// is overwritten with this token's first half. One launch replaces ~8.
// ---------------------------------------------------------------------------

__global__ void shift_decode_kernel(
    const short* __restrict__ x,     // [b, dim]
    const long* __restrict__ offset, // [1]
    short* __restrict__ ring,        // [b, S, dim/2]
    short* __restrict__ out,         // [b, dim]
    int b, int dim, int S, int text_len) {
  const int bi = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= dim) return;
  const long g0 = *offset - text_len;
  const long g = g0 < 0 ? 0 : g0;
  const int pos = (int)(g % S);
  const int prev = (int)(((g - 1) % S + S) % S);
  const int half = dim / 2, quarter = dim / 4;

  short val;
  if (i < quarter) {
    val = ring[((long)bi * S + pos) * half + i];              // top quarter
  } else if (i < half) {
    val = (g % S == 0) ? (short)0
        : ring[((long)bi * S + prev) * half + i];             // left quarter
  } else {
    val = x[(long)bi * dim + i];                              // pass-through
  }
  // race-free without a barrier: the only slot written is `pos`; element
  // ring[pos][i] is read and written by the SAME thread i (program order),
  // and the quarter..half reads touch slot `prev` != `pos` for S >= 2
  if (i < half) ring[((long)bi * S + pos) * half + i] = x[(long)bi * dim + i];
  out[(long)bi * dim + i] = val;
}

// ===========================================================================
// Host wrappers
// ===========================================================================

torch::Tensor fa_decode(torch::Tensor qkv, torch::Tensor kc, torch::Tensor vc,
                        OptTensor cosv, OptTensor sinv, torch::Tensor offset,
                        OptTensor pattern, double scale, OptTensor live,
                        OptTensor live_cnt) {
  CHK(qkv.is_cuda() && qkv.dtype() == torch::kBFloat16 && qkv.is_contiguous());
  CHK(kc.is_contiguous() && vc.is_contiguous());
  const int b = kc.size(0), h = kc.size(1), N = kc.size(2);
  CHK(kc.size(3) == 64 && N <= DEC_MAXN);
  CHK(offset.dtype() == torch::kLong);
  const RopeTables rt = rope_tables(cosv, sinv);
  const bool* pat = nullptr;
  if (pattern.has_value()) {
    CHK(pattern->dtype() == torch::kBool && pattern->is_contiguous());
    CHK(pattern->size(1) == N);
    pat = pattern->data_ptr<bool>();
  }
  auto out = torch::empty({b, (long)h * 64}, qkv.options());
  const int span = live.has_value() ? (int)live->size(1) : N;
  if (live.has_value()) {
    CHK(live->dtype() == torch::kInt32 && live->is_contiguous());
    CHK(live_cnt.has_value() && live_cnt->dtype() == torch::kInt32);
  }
  if (live.has_value() && span <= DEC_LMAX / 4) {
    // short live lists (sparse patterns): whole head in one wave, no
    // key-split scratch, no combine kernel
    hipLaunchKernelGGL(fa_decode_one_kernel, dim3((h + 3) / 4, b), dim3(256),
                       0, cur_stream(), bf16_cptr(qkv), bf16_ptr(kc),
                       bf16_ptr(vc), rt.cos, rt.sin, offset.data_ptr<long>(),
                       live->data_ptr<int>(), live_cnt->data_ptr<int>(),
                       bf16_ptr(out), b, h, N, rt.rot, (float)scale, span);
    return out;
  }
  // live lists: one 64-thread wave per 64 listed keys (no barriers);
  // scan path: 4-wave blocks over ~192-slot chunks
  int KS, chunk;
  if (live.has_value()) {
    KS = (span + 63) / 64;
    chunk = 64;
  } else {
    KS = std::min(8, std::max(2, (span + 191) / 192));
    chunk = ((span + KS - 1) / KS + 63) & ~63;
    CHK(chunk <= DEC_CHUNK_MAX);
  }
  auto scratch = torch::empty({(long)b * h * KS * 66},
                              qkv.options().dtype(torch::kFloat32));
  if (live.has_value()) {
    dim3 grid4((h + 3) / 4, b, KS);
    hipLaunchKernelGGL(fa_decode_part_list_kernel, grid4, dim3(256), 0,
                       cur_stream(), bf16_cptr(qkv), bf16_ptr(kc),
                       bf16_ptr(vc), rt.cos, rt.sin, offset.data_ptr<long>(),
                       live->data_ptr<int>(), live_cnt->data_ptr<int>(),
                       scratch.data_ptr<float>(), b, h, N, rt.rot,
                       (float)scale, KS, chunk, span);
  } else {
    hipLaunchKernelGGL(fa_decode_part_kernel, dim3(h, b, KS), dim3(256), 0,
                       cur_stream(), bf16_cptr(qkv), bf16_ptr(kc),
                       bf16_ptr(vc), rt.cos, rt.sin, offset.data_ptr<long>(),
                       pat, scratch.data_ptr<float>(), b, h, N, rt.rot,
                       (float)scale, KS, chunk);
  }
  hipLaunchKernelGGL(fa_decode_combine_kernel, dim3((h + 3) / 4, b), dim3(256),
                     0, cur_stream(), scratch.data_ptr<float>(), bf16_ptr(out),
                     b, h, KS);
  return out;
}

torch::Tensor shift_decode(torch::Tensor x, torch::Tensor offset,
                           torch::Tensor ring, int64_t text_len) {
  CHK(x.is_cuda() && x.is_contiguous() && ring.is_contiguous());
  const int b = x.size(0), dim = x.size(-1);
  const int S = ring.size(1);
  CHK(ring.size(2) == dim / 2);
  auto out = torch::empty_like(x);
  dim3 grid((dim + 255) / 256, b);
  hipLaunchKernelGGL(shift_decode_kernel, grid, dim3(256), 0, cur_stream(),
                     bf16_cptr(x), offset.data_ptr<long>(), bf16_ptr(ring),
                     bf16_ptr(out), b, dim, S, (int)text_len);
  return out;
}

TensorList dec_prelude(torch::Tensor x, OptTensor y, OptTensor scale,
                       torch::Tensor w, torch::Tensor b, OptTensor ring,
                       torch::Tensor offset, double eps, int64_t S,
                       int64_t text_len) {
  CHK(x.is_cuda() && x.dtype() == torch::kBFloat16 && x.is_contiguous());
  CHK(w.dtype() == torch::kFloat32 && b.dtype() == torch::kFloat32);
  const int dim = x.size(-1);
  const long rows = x.numel() / dim;
  const short* yp = nullptr;
  const float* sp_ = nullptr;
  torch::Tensor xn = x;
  if (y.has_value()) {
    CHK(y->is_contiguous() && scale.has_value());
    CHK(scale->dtype() == torch::kFloat32 && scale->is_contiguous());
    yp = bf16_cptr(*y);
    sp_ = scale->data_ptr<float>();
    xn = torch::empty_like(x);
  }
  short* rp = nullptr;
  if (ring.has_value()) {
    CHK(ring->dtype() == torch::kBFloat16 && ring->is_contiguous());
    rp = bf16_ptr(*ring);
  }
  auto z = torch::empty_like(x);
  dim3 grid(rows);
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, cur_stream(), bf16_cptr(x),
                       yp, sp_, w.data_ptr<float>(), b.data_ptr<float>(),
                       bf16_ptr(xn), bf16_ptr(z), rp, offset.data_ptr<long>(),
                       rows, (float)eps, (int)S, (int)text_len);
  };
  switch (dim) {
    case 512: launch(dec_prelude_kernel<2>); break;
    case 1024: launch(dec_prelude_kernel<4>); break;
    case 2048: launch(dec_prelude_kernel<8>); break;
    default: TORCH_CHECK(false, "dec_prelude: unsupported dim ", dim);
  }
  return {xn, z};
}

torch::Tensor sample_topk_gumbel(torch::Tensor logits, torch::Tensor noise,
                                 int64_t k, double temperature,
                                 OptTensor out_tok, OptTensor seq,
                                 OptTensor seq_ptr) {
  CHK(logits.is_cuda() && logits.dtype() == torch::kFloat32 &&
      logits.is_contiguous() && logits.dim() == 2);
  CHK(noise.sizes() == logits.sizes() && noise.dtype() == torch::kFloat32);
  const int rows = logits.size(0), V = logits.size(1);
  CHK(V <= 8192);
  torch::Tensor out;
  if (out_tok.has_value()) {   // write the next-token feed buffer in place
    CHK(out_tok->dtype() == torch::kLong && out_tok->is_contiguous() &&
        out_tok->numel() == rows);
    out = *out_tok;
  } else {
    out = torch::empty({rows}, logits.options().dtype(torch::kLong));
  }
  long* seqp = nullptr;
  const long* ptrp = nullptr;
  int S = 0;
  if (seq.has_value()) {
    CHK(seq_ptr.has_value() && seq_ptr->dtype() == torch::kLong);
    CHK(seq->dtype() == torch::kLong && seq->is_contiguous() &&
        seq->size(0) == rows && seq->dim() == 2);
    seqp = seq->data_ptr<long>();
    ptrp = seq_ptr->data_ptr<long>();
    S = (int)seq->size(1);
  }
  hipLaunchKernelGGL(sample_topk_gumbel_kernel, dim3(rows), dim3(256), 0,
                     cur_stream(), logits.data_ptr<float>(),
                     noise.contiguous().data_ptr<float>(),
                     out.data_ptr<long>(), seqp, ptrp, S, V, (int)k,
                     (float)(1.0 / temperature));
  return out;
}

torch::Tensor sk2(torch::Tensor x, torch::Tensor wp, OptTensor bias, long N,
                  long K, long mode, double wscale) {
  CHK(x.is_cuda() && x.dtype() == torch::kBFloat16 && x.is_contiguous());
  const bool f8 = wp.dtype() == torch::kFloat8_e4m3fn ||
                  wp.dtype() == torch::kUInt8;
  CHK((wp.dtype() == torch::kBFloat16 || f8) && wp.is_contiguous());
  const long rows = x.numel() / K;
  CHK(x.size(-1) == K);
  CHK(rows == 16 || rows == 32 || rows == 64 || rows == 128);
  // K % 1024 == 0 guarantees KCW (= K/128 chunks per wave) is a multiple of
  // every template's ring DEPTH (<= 8); smaller K would read past the last
  // chunk in the prologue
  CHK(K % 1024 == 0 && N % 32 == 0);
  CHK(wp.numel() == N * K);
  CHK(mode >= 0 && mode <= 2);
  const float* bp = nullptr;
  if (bias.has_value()) {
    CHK(bias->dtype() == torch::kFloat32 && bias->is_contiguous());
    CHK(bias->numel() == N);
    bp = bias->data_ptr<float>();
  }
  const long NO = (mode == 1) ? N / 2 : N;
  auto out = torch::empty({rows, NO},
      x.options().dtype(mode == 2 ? torch::kFloat32 : torch::kBFloat16));
  const dim3 grid(mode == 1 ? N / 32 : N / 16);
  const short* xp = bf16_cptr(x);
  const short* wpp = bf16_cptr(wp);
  void* op = out.data_ptr();
  const int Ni = (int)N, Ki = (int)K;
  // long-K bias shapes (ff2): 8-way k-split per block doubles the in-flight
  // weight stream (the 4-wave variant is HBM-latency-bound at 64 blocks)
  const bool ks8 = mode == 0 && K >= 4096 && K % 2048 == 0 && rows <= 64;
  const float ws = (float)wscale;
  #define SK2_LAUNCH(MT, MODE, KS)                                          \
    if (f8)                                                                 \
      hipLaunchKernelGGL((sk2_kernel<MT, MODE, KS, true>), grid,            \
                         dim3(KS * 64), 0, cur_stream(), xp, wpp, bp, op,   \
                         Ni, Ki, ws);                                       \
    else                                                                    \
      hipLaunchKernelGGL((sk2_kernel<MT, MODE, KS, false>), grid,           \
                         dim3(KS * 64), 0, cur_stream(), xp, wpp, bp, op,   \
                         Ni, Ki, ws)
  #define SK2_MT(MT)                                                        \
    switch (mode) {                                                         \
      case 0: if (ks8) SK2_LAUNCH(MT, 0, 8); else SK2_LAUNCH(MT, 0, 4);     \
              break;                                                        \
      case 1: SK2_LAUNCH(MT, 1, 4); break;                                  \
      default: SK2_LAUNCH(MT, 2, 4); break;                                 \
    }
  switch (rows) {
    case 16: SK2_MT(1); break;
    case 32: SK2_MT(2); break;
    case 64: SK2_MT(4); break;
    default: SK2_MT(8); break;
  }
  #undef SK2_MT
  #undef SK2_LAUNCH
  return out;
}
