// Training attention: flash attention forward (4-wave 16x16 kernel and the
// opt-in 8-wave 32x32 ladder), backward (Dv, dQ, dKdV), and the MFMA /
// permlane layout probes the tests pin those kernels' assumptions with.

#include "hip_host.h"

// ---------------------------------------------------------------------------
// Flash attention forward, head_dim = 64.
//
// Block: 256 threads = 4 waves; each block owns QBLK=64 query rows (16 per
// wave); K/V streamed in KBLK=32 tiles through LDS.
//
// "Swapped" QK^T: S^T = mfma(K_tile, Q_tile), so the MFMA C layout
// (col = lane&15, row = (lane>>4)*4 + reg) puts one query row per lane —
// softmax reduces 8 in-lane values + a 4-lane shfl_xor, no serial-lane
// section (guide §B attn / common-mistake 6). P round-trips through a
// padded LDS tile to become the PV A-fragment; V is stored transposed at
// stage time so the PV B-frag is one contiguous ds_read_b128.
// ---------------------------------------------------------------------------

constexpr int FA_QBLK = 64;     // q rows per block
constexpr int FA_KBLK = 32;     // keys per LDS tile
constexpr int FA_WAVES = 4;

constexpr int KPAD = 72;        // K tile row stride (8-elem pad -> 2-way banks)

DEVFN bf16x8 frag_from_lds(const short* base) {
  return *reinterpret_cast<const bf16x8*>(base);  // ds_read_b128
}

// Block-XOR swizzle for the transposed LDS tiles ([64 d][64 keys(+pad)]):
// XOR the key's 8-block index with the d-row's block index. Without it,
// every 16-byte-aligned row stride puts all d-blocks of one key group in
// the same banks, so the 8-element scalar transpose-stores serialize
// 8-way (PMC: 88M SQ_LDS_BANK_CONFLICT per fa_fwd dispatch). The XOR
// flips only key bits 3..5, so 8-element groups stay contiguous and the
// ds_read_b128 fragments remain 16B-aligned.
DEVFN int swz_key(int d, int key) {
  return key ^ (((d >> 3) & 7) << 3);
}

// ---------------------------------------------------------------------------
// Axial attention mode (reference attention.py:225-335): instead of a
// static mask in HBM + tile maps, the axial pattern is evaluated
// ARITHMETICALLY in a virtual coordinate space. Virtual rows 0..n-1 are the
// text prefix (identity) followed by the image grid in row-major order for
// axis 0 or COLUMN-major order for axis 1 — so the "own grid line" of every
// query is a contiguous virtual key range for both axes, and axis 1 needs
// no tensor transposes (keys are fetched through the row map; each key row
// is a contiguous 128 B line either way). Liveness: text keys are visible
// to everything causal; image keys only within the same grid line, causal.
// ---------------------------------------------------------------------------

DEVFN int ax_phys(int vrow, int t, int logS, int axis) {
  if (axis != 1 || vrow < t) return vrow;
  const int i = vrow - t;
  return t + ((i & ((1 << logS) - 1)) << logS) + (i >> logS);
}

DEVFN bool ax_ok(int vq, int vk, int t, int logS) {
  if (vk < t) return vq < t ? vk <= vq : true;
  if (vq < vk || vq < t) return false;
  return ((vq - t) >> logS) == ((vk - t) >> logS);
}

// XCD-aware block mapping (guide T1, bijective m204 form): the runtime
// round-robins flat block ids across the 8 XCDs, so consecutive ids land on
// different L2s. Remapping gives each XCD a CONTIGUOUS range of the
// (bh-major) linearization — q-tiles that share one (batch,head)'s K/V
// stream stay on one XCD's L2 instead of re-fetching from HBM 8x.
DEVFN void xcd_chunked(int bid, int nwg, int tiles_per_bh,
                       int* tile, int* bh) {
  constexpr int NXCD = 8;
  const int q = nwg / NXCD, r = nwg % NXCD;
  const int xcd = bid % NXCD, pos = bid / NXCD;
  const int lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + pos;
  *tile = lin % tiles_per_bh;
  *bh = lin / tiles_per_bh;
}

// ---- (64, 32) tile-map helpers shared by the forward, dQ and dKdV kernels.
// The host precomputes, per (64 block rows, 32 streamed rows) granule,
// whether any static-mask entry is set (1) or all of them are (2); a block's
// map row has one byte per granule, and a 64-row compute tile spans two.

// stage the block's tile-map row in LDS (`lds`, 128 bytes): the sequential
// next_live scan otherwise pays a full vmcnt(0) round-trip per granule byte
// (ISA-verified ~0.7 us per scanned tile on the conv/block-sparse configs)
DEVFN const unsigned char* stage_tmap_row(const unsigned char* tmap_row,
                                          int ng, unsigned char* lds) {
  if (tmap_row != nullptr && ng <= 128) {
    for (int i = threadIdx.x; i < ng; i += blockDim.x)
      lds[i] = tmap_row[i];
    __syncthreads();
    tmap_row = lds;
  }
  return tmap_row;
}

// block-sparse skip: a 64-row tile is live if either of its granules is
// (axial/conv/block-sparse patterns)
DEVFN bool tmap_pair_live(const unsigned char* tmap_row, int t, int ng) {
  const int g0 = 2 * t;
  bool live = tmap_row[g0] != 0;
  if (g0 + 1 < ng) live |= tmap_row[g0 + 1] != 0;
  return live;
}

// a tile whose two map granules are both 2 has every mask entry set:
// combined with causal-interior + bounds checks the per-element mask
// loop can be skipped (the fa kernels are VALU-bound on exactly that)
DEVFN bool tmap_pair_full(const unsigned char* tmap_row, int t, int ng) {
  const int g0 = 2 * t;
  if (g0 + 1 >= ng) return false;
  return tmap_row[g0] == 2 && tmap_row[g0 + 1] == 2;
}

__global__ __launch_bounds__(256, 2)
void fa_fwd_d64_kernel(
    const short* __restrict__ q,    // [bh, nq, 64] bf16 bits
    const short* __restrict__ k,    // [bh, nk, 64]
    const short* __restrict__ v,    // [bh, nk, 64]
    short* __restrict__ out,        // [bh, nq, 64], or [b, nq, h, 64] if out_bnhd
    float* __restrict__ lse,        // [bh, nq]
    const bool* __restrict__ key_mask,    // [b, nk] or null
    const bool* __restrict__ static_mask, // [nq, nk] or null
    const unsigned char* __restrict__ tile_map,  // [ceil(nq/64), ceil(nk/32)] or null
    int b, int h, int nq, int nk,
    float scale, int causal, int out_bnhd,
    int ax_t, int ax_logS, int ax_axis) {        // axial mode if ax_axis >= 0

  // KV tiles are 64 keys (2 map granules); staging is software-pipelined:
  // the next live tile's global loads are issued before this tile's MFMA
  // work so HBM latency hides under the compute (guide G15 async-STAGE).
  constexpr int KV = 2 * FA_KBLK;             // 64 keys per LDS tile
  __shared__ short Kt[KV][KPAD];
  __shared__ short Vt[FA_D][KV + 8];
  __shared__ short Pl[FA_WAVES][16][KV + 8];
  __shared__ unsigned char Mtile[FA_QBLK][KV + 16];   // static-mask tile (80B stride: 2-way reads)

  const int n_qt = (nq + FA_QBLK - 1) / FA_QBLK;
  int qtile, bh;
  xcd_chunked(blockIdx.x, n_qt * b * h, n_qt, &qtile, &bh);
  const int batch = bh / h;
  const int q0 = qtile * FA_QBLK;
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int lq = lane & 15;       // this lane's query row within the wave tile
  const int grp = lane >> 4;      // lane group 0..3

  const int qrow = q0 + wave * 16 + lq;   // this lane's global query row
  const int diag = nk - nq;               // causal offset (ref triu(j-i+1))

  const bool axial = ax_axis >= 0;
  const short* qp = q + (long)bh * nq * FA_D;
  const short* kp = k + (long)bh * nk * FA_D;
  const short* vp = v + (long)bh * nk * FA_D;

  // Q fragments (B-operand of the swapped QK^T):
  // lane holds Q[lq][8*grp + e + 32*c], c = 0,1
  const int qphys = axial ? ax_phys(qrow, ax_t, ax_logS, ax_axis) : qrow;
  // first key of this q row's own grid line (INT_MAX for text rows): the
  // axial element test reduces to 4 branchless compares
  const int ax_klo = (axial && qrow < nq && qrow >= ax_t)
      ? ax_t + (((qrow - ax_t) >> ax_logS) << ax_logS) : 0x7fffffff;
  bf16x8 qfrag[2];
  {
    const bool qok = qrow < nq;
    #pragma unroll
    for (int c = 0; c < 2; ++c) {
      qfrag[c] = qok
          ? *reinterpret_cast<const bf16x8*>(qp + (long)qphys * FA_D + 8 * grp + 32 * c)
          : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }

  // exp2-domain softmax: exp(x) lowers to v_exp_f32(x*log2e) on gfx9+, so
  // folding log2e into the score scale (a multiply that happens anyway)
  // saves one VALU mul per score element in kernels measured 92-96%
  // VALU-bound (profiles/pmc_final_r2.txt); lse converts back to natural
  // log once per row at the write (the external contract is unchanged)
  const float scl2 = scale * 1.44269504088896f;
  float m_run = NEG_INF;   // per-q-row online-softmax state (q = lq)
  float l_run = 0.f;
  f32x4 acc[4] = {f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0},
                  f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0}};

  const int ntk = (nk + FA_KBLK - 1) / FA_KBLK;   // 32-key map granules
  int ntiles = (nk + KV - 1) / KV;                // 64-key compute tiles
  if (causal) {
    const int lim = min(nk - 1, q0 + FA_QBLK - 1 + diag);
    ntiles = lim < 0 ? 0 : (lim / KV + 1);
  }
  __shared__ unsigned char TMrow[128];
  const unsigned char* tmap_row = stage_tmap_row(
      tile_map ? tile_map + (long)qtile * ntk : nullptr, ntk, TMrow);

  // In axial mode liveness is pure arithmetic: text tiles always, image
  // tiles only when they overlap the q-block's own grid-line span.
  auto tile_live = [&](int t) -> bool {
    if (axial) {
      const int kbase = t * KV;
      if (kbase < ax_t) return true;
      if (q0 + FA_QBLK <= ax_t) return false;
      const int l0 = (max(q0, ax_t) - ax_t) >> ax_logS;
      return kbase + KV > ax_t + (l0 << ax_logS);
    }
    return !tmap_row || tmap_pair_live(tmap_row, t, ntk);
  };
  auto next_live = [&](int t) -> int {
    while (t < ntiles && !tile_live(t)) ++t;
    return t;
  };

  // staging geometry: 64 rows x 64 cols = 512 16B chunks, 2 per thread
  const int srow0 = tid >> 3;           // chunk-0 row (0..31)
  const int sc8 = (tid & 7) * 8;        // chunk col
  int4v kreg[2], vreg[2], mreg;
  // mask staging: 64x64 bytes = one 16B chunk per thread
  const int mrow = tid >> 2;            // 0..63
  const int mc16 = (tid & 3) * 16;

  auto prefetch = [&](int t) {
    const int kbase = t * KV;
    #pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int kg = kbase + srow0 + 32 * half;
      if (kg < nk) {
        const int kph = axial ? ax_phys(kg, ax_t, ax_logS, ax_axis) : kg;
        kreg[half] = *reinterpret_cast<const int4v*>(kp + (long)kph * FA_D + sc8);
        vreg[half] = *reinterpret_cast<const int4v*>(vp + (long)kph * FA_D + sc8);
      } else {
        kreg[half] = int4v{0, 0, 0, 0};
        vreg[half] = int4v{0, 0, 0, 0};
      }
    }
    if (static_mask != nullptr) {
      const int mq = q0 + mrow;
      const long base = (long)mq * nk + kbase + mc16;
      if (mq < nq && kbase + mc16 + 16 <= nk && (base & 15) == 0) {
        mreg = *reinterpret_cast<const int4v*>(
            reinterpret_cast<const char*>(static_mask) + base);
      } else {
        unsigned char mb[16];
        #pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int kg = kbase + mc16 + e;
          mb[e] = (mq < nq && kg < nk)
              ? (unsigned char)static_mask[(long)mq * nk + kg] : 0;
        }
        mreg = *reinterpret_cast<const int4v*>(mb);
      }
    }
  };

  int kt = next_live(0);
  if (kt < ntiles) prefetch(kt);

  while (kt < ntiles) {
    const int kbase = kt * KV;
    const int kt_next = next_live(kt + 1);

    __syncthreads();   // prior tile fully consumed before overwrite
    #pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int row = srow0 + 32 * half;
      *reinterpret_cast<int4v*>(&Kt[row][sc8]) = kreg[half];
      const short* vs = reinterpret_cast<const short*>(&vreg[half]);
      #pragma unroll
      for (int e = 0; e < 8; ++e)
        Vt[sc8 + e][swz_key(sc8 + e, row)] = vs[e];
    }
    if (static_mask != nullptr)
      *reinterpret_cast<int4v*>(&Mtile[mrow][mc16]) = mreg;
    __syncthreads();

    // issue the NEXT tile's loads now: HBM latency hides under the MFMA +
    // softmax work below
    if (kt_next < ntiles) prefetch(kt_next);

    // ---- swapped QK^T: four 16-key subtiles, contraction K=64 in 2 steps
    float s16[16];
    __builtin_amdgcn_s_setprio(1);
    #pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      f32x4 st{0, 0, 0, 0};
      #pragma unroll
      for (int c = 0; c < 2; ++c) {
        bf16x8 af = frag_from_lds(&Kt[mt * 16 + lq][8 * grp + 32 * c]);
        st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, qfrag[c], st, 0, 0, 0);
      }
      #pragma unroll
      for (int r = 0; r < 4; ++r) s16[mt * 4 + r] = st[r];
    }
    __builtin_amdgcn_s_setprio(0);
    // After the swap: C col = lane&15 = q row; C row = grp*4 + r = key.
    // s16[i] = S[qrow][kbase + (i>>2)*16 + grp*4 + (i&3)].

    // ---- scale + masks (uniform fast path for fully-unmasked interior)
    const bool interior = key_mask == nullptr &&
        (q0 + FA_QBLK <= nq) && (kbase + KV <= nk) &&
        (axial
             ? ((q0 >= ax_t && kbase + KV <= ax_t) ||        // img q x text k
                (q0 + FA_QBLK <= ax_t && kbase + KV - 1 <= q0))  // text causal
             : ((!causal || (kbase + KV - 1 <= q0 + diag)) &&
                (static_mask == nullptr ||
                 (tmap_row != nullptr && tmap_pair_full(tmap_row, kt, ntk)))));
    if (interior) {
      #pragma unroll
      for (int i = 0; i < 16; ++i) s16[i] *= scl2;
    } else if (axial) {
      #pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int kg = kbase + (i >> 2) * 16 + grp * 4 + (i & 3);
        bool ok = (kg < nk) & (qrow < nq) & (kg <= qrow) &
                  ((kg < ax_t) | (kg >= ax_klo));
        if (key_mask != nullptr && ok)
          ok &= key_mask[(long)batch * nk + ax_phys(kg, ax_t, ax_logS, ax_axis)];
        s16[i] = ok ? s16[i] * scl2 : NEG_INF;
      }
    } else {
      #pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int kg = kbase + (i >> 2) * 16 + grp * 4 + (i & 3);
        bool ok = (kg < nk) & (qrow < nq);
        if (causal) ok &= kg <= qrow + diag;
        if (key_mask != nullptr && ok) ok &= key_mask[(long)batch * nk + kg];
        if (static_mask != nullptr && ok)
          ok &= Mtile[wave * 16 + lq][kg - kbase] != 0;
        s16[i] = ok ? s16[i] * scl2 : NEG_INF;
      }
    }

    // ---- online softmax update (lane-local + 4-lane reduce per q row)
    float mt_part = NEG_INF;
    #pragma unroll
    for (int i = 0; i < 16; ++i) mt_part = fmaxf(mt_part, s16[i]);
    mt_part = fmaxf(mt_part, __shfl_xor(mt_part, 16));
    mt_part = fmaxf(mt_part, __shfl_xor(mt_part, 32));

    // defer-max (guide T13): if no row's max grew by more than 8, keep the
    // old running max — P stays bounded by e^8 and the O-rescale is skipped
    const bool defer = __all(mt_part <= m_run + 11.5416f);  // 8 nats
    const float m_new = defer ? m_run : fmaxf(m_run, mt_part);

    float lsum = 0.f;
    float p16[16];
    #pragma unroll
    for (int i = 0; i < 16; ++i) {
      p16[i] = (s16[i] == NEG_INF) ? 0.f : fexp2(s16[i] - m_new);
      lsum += p16[i];
    }
    lsum += __shfl_xor(lsum, 16);
    lsum += __shfl_xor(lsum, 32);

    float alpha = 1.f;
    if (!defer) {
      alpha = (m_run == NEG_INF) ? 0.f : fexp2(m_run - m_new);
      if (m_new != NEG_INF) m_run = m_new;
    }
    l_run = l_run * alpha + lsum;

    // ---- P -> LDS (bf16) to reshape into the PV A-fragment; each quarter
    // lands at 4 consecutive kk, so pack into one 8-byte store
    #pragma unroll
    for (int a = 0; a < 4; ++a) {
      bf16x4 pk;
      #pragma unroll
      for (int e = 0; e < 4; ++e) pk[e] = f2bf(p16[a * 4 + e]);
      *reinterpret_cast<bf16x4*>(&Pl[wave][lq][16 * a + 4 * grp]) = pk;
    }

    if (!defer) {
      // rescale accumulators; acc rows are q = grp*4 + r, alphas live on
      // lanes whose (lane&15) equals that q row
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float a_r = __shfl(alpha, grp * 4 + r);
        #pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[nt][r] *= a_r;
      }
    }

    // ---- PV: contraction over this tile's 64 keys in two 32-key steps
    bf16x8 pf0 = frag_from_lds(&Pl[wave][lq][8 * grp]);
    bf16x8 pf1 = frag_from_lds(&Pl[wave][lq][32 + 8 * grp]);
    __builtin_amdgcn_s_setprio(1);
    #pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int d = lq + 16 * nt;
      bf16x8 vf0 = frag_from_lds(&Vt[d][swz_key(d, 8 * grp)]);
      bf16x8 vf1 = frag_from_lds(&Vt[d][swz_key(d, 32 + 8 * grp)]);
      acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf0, vf0, acc[nt], 0, 0, 0);
      acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf1, vf1, acc[nt], 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);

    kt = kt_next;
  }

  // ---- epilogue: divide by l per q row, store out + lse. out_bnhd writes
  // the [b, n, h*d] layout directly so no head-merge permute kernel is
  // needed before the output projection GEMM.
  const int batch_i = bh / h, head_i = bh - batch_i * h;
  #pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qr = q0 + wave * 16 + grp * 4 + r;
    const float l_r = __shfl(l_run, grp * 4 + r);
    const float inv = l_r > 0.f ? 1.f / l_r : 0.f;
    if (qr < nq) {
      const int qrp = axial ? ax_phys(qr, ax_t, ax_logS, ax_axis) : qr;
      const long base = out_bnhd
          ? (((long)batch_i * nq + qrp) * h + head_i) * FA_D
          : ((long)bh * nq + qrp) * FA_D;
      #pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        out[base + 16 * nt + lq] = f2bf(acc[nt][r] * inv);
      }
    }
  }
  if (grp == 0 && qrow < nq) {
    lse[(long)bh * nq + qphys] = (l_run > 0.f)
        ? (m_run + __log2f(l_run)) * 0.69314718055995f : NEG_INF;
  }
}

// ---------------------------------------------------------------------------
// 8-wave 32x32 MFMA attention forward ("fa8 ladder", guide §B attn /
// NOTES_ROUND2 item 1, layouts machine-checked by scripts/plan_fa8.py +
// tests/test_fa8_plan.py). Block = 8 waves x 32 q rows = 256 q rows;
// KV staged in 64-key LDS tiles. Per wave everything stays in registers:
// swapped QK^T (mfma(K, Q^T) -> S^T with q = lane&31 lane-local), 15-op
// in-lane + 1 permlane32_swap row reduces, defer-max online softmax, P
// packed to bf16 pairs and redistributed across the lane halves with 8
// permlane32_swaps per tile (no P LDS round-trip), PV from the transposed
// V tile. Covers dense causal/non-causal, key_mask, and axial mode; the
// masked/tile-map patterns stay on the 4-wave 16x16 kernel.
// ---------------------------------------------------------------------------

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int FA8_QBLK = 256;
constexpr int FA8_KV = 64;

// K tile [64 keys][64 d] bf16 at 128 B rows; byte ^= (row&3)<<5 floors both
// the 16 B-chunk store and the b128 A-fragment read (plan_fa8 d64_swizzle)
DEVFN short* k8_addr(short* base, int row, int byte) {
  return reinterpret_cast<short*>(
      reinterpret_cast<char*>(base) + ((row * 128 + byte) ^ ((row & 3) << 5)));
}

DEVFN unsigned pk_bf16(float a, float b) {
  // native casts pair into one v_cvt_pk_bf16_f32 (guide T12/m240: the
  // compiler's pick beats both hand asm and a manual RNE bit-trick here)
  union { __bf16 h[2]; unsigned u; } c;
  c.h[0] = (__bf16)a;
  c.h[1] = (__bf16)b;
  return c.u;
}

// value of `w` in lane (lane ^ 32): one v_permlane32_swap_b32, result
// element picked per half (semantics pinned by test_permlane_semantics)
DEVFN unsigned partner_u32(unsigned w, bool hi_half) {
  auto r = __builtin_amdgcn_permlane32_swap(w, w, false, false);
  return hi_half ? r[0] : r[1];
}

DEVFN float partner_f32(float v, bool hi_half) {
  union { float f; unsigned u; } c;
  c.f = v;
  c.u = partner_u32(c.u, hi_half);
  return c.f;
}

__global__ __launch_bounds__(512, 2)
void fa8_fwd_d64_kernel(
    const short* __restrict__ q,    // [bh, nq, 64] bf16 bits
    const short* __restrict__ k,    // [bh, nk, 64]
    const short* __restrict__ v,    // [bh, nk, 64]
    short* __restrict__ out,        // [bh, nq, 64] or [b, nq, h, 64]
    float* __restrict__ lse,        // [bh, nq]
    const bool* __restrict__ key_mask,   // [b, nk] or null
    int b, int h, int nq, int nk,
    float scale, int causal, int out_bnhd,
    int ax_t, int ax_logS, int ax_axis) {

  __shared__ short K8[64 * 64];
  __shared__ short V8t[64][FA8_KV + 8];
  __shared__ float bcast[8][32];

  const int n_qt = (nq + FA8_QBLK - 1) / FA8_QBLK;
  int qtile, bh;
  xcd_chunked(blockIdx.x, n_qt * b * h, n_qt, &qtile, &bh);
  const int batch = bh / h;
  const int q0 = qtile * FA8_QBLK;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int lq = lane & 31;              // this lane's q row within the wave
  const int half = lane >> 5;            // lane half (0/1)
  const int qrow = q0 + wave * 32 + lq;
  const int diag = nk - nq;
  const bool axial = ax_axis >= 0;
  const int qphys = axial ? ax_phys(qrow, ax_t, ax_logS, ax_axis) : qrow;

  const short* qp = q + (long)bh * nq * FA_D;
  const short* kp = k + (long)bh * nk * FA_D;
  const short* vp = v + (long)bh * nk * FA_D;

  // Q fragments (B operand): lane holds Q[q = lane&31][16c + 8*half + e]
  bf16x8 qfrag[4];
  {
    const bool qok = qrow < nq;
    #pragma unroll
    for (int c = 0; c < 4; ++c) {
      qfrag[c] = qok
          ? *reinterpret_cast<const bf16x8*>(
                qp + (long)qphys * FA_D + 16 * c + 8 * half)
          : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }

  const float scl2 = scale * 1.44269504088896f;
  float m_run = NEG_INF, l_run = 0.f;
  f32x16 acc_o[2] = {};
  const int wave_qmax = q0 + wave * 32 + 31 + diag;   // causal bound

  int ntiles = (nk + FA8_KV - 1) / FA8_KV;
  if (causal) {
    const int lim = min(nk - 1, q0 + FA8_QBLK - 1 + diag);
    ntiles = lim < 0 ? 0 : (lim / FA8_KV + 1);
  }
  auto tile_live_blk = [&](int t) -> bool {
    if (!axial) return true;
    const int kbase = t * FA8_KV;
    if (kbase < ax_t) return true;
    if (q0 + FA8_QBLK <= ax_t) return false;
    const int l0 = (max(q0, ax_t) - ax_t) >> ax_logS;
    return kbase + FA8_KV > ax_t + (l0 << ax_logS);
  };
  auto next_live = [&](int t) -> int {
    while (t < ntiles && !tile_live_blk(t)) ++t;
    return t;
  };

  // staging: 512 threads x 16 B = one 64x128 B tile per pass
  const int srow = tid >> 3;
  const int sc8 = (tid & 7) * 8;
  int4v kreg, vreg;
  auto prefetch = [&](int t) {
    const int kg = t * FA8_KV + srow;
    if (kg < nk) {
      const int kph = axial ? ax_phys(kg, ax_t, ax_logS, ax_axis) : kg;
      kreg = *reinterpret_cast<const int4v*>(kp + (long)kph * FA_D + sc8);
      vreg = *reinterpret_cast<const int4v*>(vp + (long)kph * FA_D + sc8);
    } else {
      kreg = int4v{0, 0, 0, 0};
      vreg = int4v{0, 0, 0, 0};
    }
  };

  int kt = next_live(0);
  if (kt < ntiles) prefetch(kt);

  while (kt < ntiles) {
    const int kbase = kt * FA8_KV;
    const int kt_next = next_live(kt + 1);

    __syncthreads();
    *reinterpret_cast<int4v*>(k8_addr(K8, srow, sc8 * 2)) = kreg;
    {
      const short* vs = reinterpret_cast<const short*>(&vreg);
      #pragma unroll
      for (int e = 0; e < 8; ++e)
        V8t[sc8 + e][swz_key(sc8 + e, srow)] = vs[e];
    }
    __syncthreads();
    if (kt_next < ntiles) prefetch(kt_next);

    const bool wave_dead = causal && kbase > wave_qmax;
    if (!wave_dead) {
      // ---- swapped QK^T: two 32-key subtiles, contraction K=64 in 4 mfmas
      f32x16 acc_s[2] = {};
      __builtin_amdgcn_s_setprio(1);
      #pragma unroll
      for (int s = 0; s < 2; ++s) {
        #pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int row = 32 * s + lq;
          const bf16x8 af = *reinterpret_cast<const bf16x8*>(
              k8_addr(K8, row, (16 * c + 8 * half) * 2));
          acc_s[s] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              af, qfrag[c], acc_s[s], 0, 0, 0);
        }
      }
      __builtin_amdgcn_s_setprio(0);

      // ---- scale + masks. Element (s, r): key = kbase + 32 s + crow(r),
      // q = qrow, with crow(r) = (r&3) + 8*(r>>2) + 4*half.
      const bool interior = key_mask == nullptr &&
          (kbase + FA8_KV <= nk) && (qrow < nq) &&
          (axial
               ? ((q0 >= ax_t && kbase + FA8_KV <= ax_t) ||
                  (q0 + FA8_QBLK <= ax_t && kbase + FA8_KV - 1 <= qrow &&
                   kbase + FA8_KV - 1 <= q0 + wave * 32 + diag))
               : (!causal || kbase + FA8_KV - 1 <= q0 + wave * 32 + diag));
      float s32[32];
      if (interior) {
        #pragma unroll
        for (int s = 0; s < 2; ++s)
          #pragma unroll
          for (int r = 0; r < 16; ++r) s32[16 * s + r] = acc_s[s][r] * scl2;
      } else {
        #pragma unroll
        for (int s = 0; s < 2; ++s) {
          #pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = kbase + 32 * s + (r & 3) + 8 * (r >> 2) + 4 * half;
            bool ok = (key < nk) & (qrow < nq);
            if (axial) {
              ok = ok && ax_ok(qrow, key, ax_t, ax_logS);
            } else if (causal) {
              ok &= key <= qrow + diag;
            }
            if (key_mask != nullptr && ok) {
              const int kph = axial ? ax_phys(key, ax_t, ax_logS, ax_axis) : key;
              ok &= key_mask[(long)batch * nk + kph];
            }
            s32[16 * s + r] = ok ? acc_s[s][r] * scl2 : NEG_INF;
          }
        }
      }

      // ---- online softmax: 31-value in-lane max + one permlane32_swap
      float mt = NEG_INF;
      #pragma unroll
      for (int i = 0; i < 32; ++i) mt = fmaxf(mt, s32[i]);
      mt = fmaxf(mt, partner_f32(mt, half));

      const bool defer = __all(mt <= m_run + 11.5416f);
      const float m_new = defer ? m_run : fmaxf(m_run, mt);

      float p32[32];
      float lsum = 0.f;
      #pragma unroll
      for (int i = 0; i < 32; ++i) {
        p32[i] = (s32[i] == NEG_INF) ? 0.f : fexp2(s32[i] - m_new);
        lsum += p32[i];
      }
      lsum += partner_f32(lsum, half);

      float alpha = 1.f;
      if (!defer) {
        alpha = (m_run == NEG_INF) ? 0.f : fexp2(m_run - m_new);
        if (m_new != NEG_INF) m_run = m_new;
        // alpha is per q (= lane&31); the PV accumulator rows are crow(r)
        // -> broadcast through this wave's 32-slot LDS row
        if (lane < 32) bcast[wave][lq] = alpha;
        #pragma unroll
        for (int d0 = 0; d0 < 2; ++d0) {
          #pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int qr = (r & 3) + 8 * (r >> 2) + 4 * half;
            acc_o[d0][r] *= bcast[wave][qr];
          }
        }
      }
      l_run = l_run * alpha + lsum;

      // ---- P -> bf16 pairs, partner halves fetched with permlane32_swap
      // (plan_fa8 p_value map). A-frag for key slice ks: rbase = 4*(2*(ks&1)
      // + half) in subtile ks>>1; [own 4 | partner 4] ordered by half.
      // Every lane packs BOTH register groups of the slice — LOW (regs
      // 8t..8t+3: the h=0 frag's domain) and HIGH (8t+4..8t+7: h=1's) —
      // and ONE permlane32_swap(wL, wH) hands each half exactly the
      // partner word it needs (r[1].lo = partner LOW for h=0, r[0].hi =
      // partner HIGH for h=1): 8 cvt-packs + 2 swaps per 16-key slice.
      bf16x8 paf[4];
      #pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const float* ps = &p32[16 * (ks >> 1)];
        const int rL = 8 * (ks & 1);
        const unsigned wL0 = pk_bf16(ps[rL], ps[rL + 1]);
        const unsigned wL1 = pk_bf16(ps[rL + 2], ps[rL + 3]);
        const unsigned wH0 = pk_bf16(ps[rL + 4], ps[rL + 5]);
        const unsigned wH1 = pk_bf16(ps[rL + 6], ps[rL + 7]);
        auto rA = __builtin_amdgcn_permlane32_swap(wL0, wH0, false, false);
        auto rB = __builtin_amdgcn_permlane32_swap(wL1, wH1, false, false);
        unsigned fr[4];
        if (half == 0) {
          fr[0] = wL0; fr[1] = wL1; fr[2] = rA[1]; fr[3] = rB[1];
        } else {
          fr[0] = rA[0]; fr[1] = rB[0]; fr[2] = wH0; fr[3] = wH1;
        }
        paf[ks] = *reinterpret_cast<const bf16x8*>(fr);
      }

      // ---- PV over the transposed V tile
      __builtin_amdgcn_s_setprio(1);
      #pragma unroll
      for (int d0 = 0; d0 < 2; ++d0) {
        const int d = 32 * d0 + lq;
        #pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const bf16x8 vf = frag_from_lds(
              &V8t[d][swz_key(d, 16 * ks + 8 * half)]);
          acc_o[d0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              paf[ks], vf, acc_o[d0], 0, 0, 0);
        }
      }
      __builtin_amdgcn_s_setprio(0);
    }

    kt = kt_next;
  }

  // ---- epilogue: normalize rows by l_run[qrow] (LDS broadcast), store
  if (lane < 32) bcast[wave][lq] = l_run > 0.f ? 1.f / l_run : 0.f;
  const int batch_i = bh / h, head_i = bh - batch_i * h;
  #pragma unroll
  for (int d0 = 0; d0 < 2; ++d0) {
    #pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qr_loc = (r & 3) + 8 * (r >> 2) + 4 * half;
      const int qr = q0 + wave * 32 + qr_loc;
      if (qr < nq) {
        const int qrp = axial ? ax_phys(qr, ax_t, ax_logS, ax_axis) : qr;
        const long base = out_bnhd
            ? (((long)batch_i * nq + qrp) * h + head_i) * FA_D
            : ((long)bh * nq + qrp) * FA_D;
        out[base + 32 * d0 + lq] = f2bf(acc_o[d0][r] * bcast[wave][qr_loc]);
      }
    }
  }
  if (lane < 32 && qrow < nq) {
    lse[(long)bh * nq + qphys] = (l_run > 0.f)
        ? (m_run + __log2f(l_run)) * 0.69314718055995f : NEG_INF;
  }
}

// probe for v_permlane32_swap_b32 result-element semantics (consumed by
// tests/test_gpu_kernels.py::test_permlane_semantics)
__global__ void permlane_probe_kernel(const unsigned* __restrict__ a,
                                      const unsigned* __restrict__ bsrc,
                                      unsigned* __restrict__ r0,
                                      unsigned* __restrict__ r1) {
  const unsigned va = a[threadIdx.x], vb = bsrc[threadIdx.x];
  auto r = __builtin_amdgcn_permlane32_swap(va, vb, false, false);
  r0[threadIdx.x] = r[0];
  r1[threadIdx.x] = r[1];
}

// ---------------------------------------------------------------------------
// Flash attention backward, head_dim = 64 (two passes, standard flash
// decomposition — no n x n matrix in HBM):
//   D[q]   = rowsum(dO * O)                       (host-side fused reduce)
//   P      = exp(scale*QK^T - lse)  (masked -> 0) (recomputed per tile)
//   dV     = P^T dO;   dP = dO V^T
//   dS     = P * (dP - D) * scale
//   dQ     = dS K;     dK = dS^T Q
// Pass 1 (dq): blocks own 64 q rows, stream K/V tiles — same swapped-MFMA
// structure as the forward. Pass 2 (dkv): blocks own 64 keys, stream Q/dO
// tiles with the roles mirrored. Both honor the causal bound and the
// (64,32) tile maps, so sparse patterns stay sparse in backward too.
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256, 2)
void fa_bwd_dq_kernel(
    const short* __restrict__ q,     // [bh, nq, 64]
    const short* __restrict__ k,     // [bh, nk, 64]
    const short* __restrict__ v,     // [bh, nk, 64]
    const short* __restrict__ dout,  // [bh, nq, 64]
    const float* __restrict__ lse,   // [bh, nq]
    const float* __restrict__ Dv,    // [bh, nq]
    short* __restrict__ dq,          // [bh, nq, 64]
    const bool* __restrict__ key_mask,
    const bool* __restrict__ static_mask,
    const unsigned char* __restrict__ tile_map,   // [nq/64, nk/32]
    int b, int h, int nq, int nk, float scale, int causal, int do_bnhd,
    int ax_t, int ax_logS, int ax_axis) {

  constexpr int KV = 2 * FA_KBLK;          // 64 keys per LDS tile
  __shared__ short Kt[KV][KPAD];           // K row-major
  __shared__ short Vr[KV][KPAD];           // V row-major (A-operand of dP^T)
  __shared__ short Ktr[FA_D][KV + 8];      // K transposed (B-operand of dS*K)
  __shared__ short DSl[FA_WAVES][16][KV + 8];
  __shared__ unsigned char Mtile[FA_QBLK][KV + 16];

  const int n_qt = (nq + FA_QBLK - 1) / FA_QBLK;
  int qtile, bh;
  xcd_chunked(blockIdx.x, n_qt * b * h, n_qt, &qtile, &bh);
  const int batch = bh / h;
  const int q0 = qtile * FA_QBLK;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int lq = lane & 15, grp = lane >> 4;
  const int qrow = q0 + wave * 16 + lq;
  const int diag = nk - nq;

  const short* qp = q + (long)bh * nq * FA_D;
  const short* kp = k + (long)bh * nk * FA_D;
  const short* vp = v + (long)bh * nk * FA_D;
  const long do_stride = do_bnhd ? (long)h * FA_D : FA_D;
  const short* dop = do_bnhd
      ? dout + ((long)batch * nq * h + (bh - batch * h)) * FA_D
      : dout + (long)bh * nq * FA_D;

  const bool axial = ax_axis >= 0;
  const int qphys = axial ? ax_phys(qrow, ax_t, ax_logS, ax_axis) : qrow;
  const int ax_klo = (axial && qrow < nq && qrow >= ax_t)
      ? ax_t + (((qrow - ax_t) >> ax_logS) << ax_logS) : 0x7fffffff;
  bf16x8 qfrag[2], dofrag[2];
  const float scl2 = scale * 1.44269504088896f;
  float lse_q = 0.f, D_q = 0.f;
  {
    const bool qok = qrow < nq;
    #pragma unroll
    for (int c = 0; c < 2; ++c) {
      qfrag[c] = qok ? *reinterpret_cast<const bf16x8*>(qp + (long)qphys * FA_D + 8 * grp + 32 * c)
                     : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      dofrag[c] = qok ? *reinterpret_cast<const bf16x8*>(dop + (long)qphys * do_stride + 8 * grp + 32 * c)
                      : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
    if (qok) {
      // exp2-domain: p = exp2(s*scl2 - lse*log2e); ds keeps natural scale
      lse_q = lse[(long)bh * nq + qphys] * 1.44269504088896f;
      D_q = Dv[(long)bh * nq + qphys];
    }
  }

  f32x4 acc[4] = {f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0},
                  f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0}};

  const int ntk = (nk + FA_KBLK - 1) / FA_KBLK;
  int ntiles = (nk + KV - 1) / KV;
  if (causal) {
    const int lim = min(nk - 1, q0 + FA_QBLK - 1 + diag);
    ntiles = lim < 0 ? 0 : (lim / KV + 1);
  }
  __shared__ unsigned char TMrow[128];
  const unsigned char* tmap_row = stage_tmap_row(
      tile_map ? tile_map + (long)qtile * ntk : nullptr, ntk, TMrow);

  auto tile_live = [&](int t) -> bool {
    if (axial) {
      const int kbase = t * KV;
      if (kbase < ax_t) return true;
      if (q0 + FA_QBLK <= ax_t) return false;
      const int l0 = (max(q0, ax_t) - ax_t) >> ax_logS;
      return kbase + KV > ax_t + (l0 << ax_logS);
    }
    return !tmap_row || tmap_pair_live(tmap_row, t, ntk);
  };
  auto next_live = [&](int t) -> int {
    while (t < ntiles && !tile_live(t)) ++t;
    return t;
  };

  const int srow0 = tid >> 3;
  const int sc8 = (tid & 7) * 8;
  const int mrow = tid >> 2;
  const int mc16 = (tid & 3) * 16;
  int4v kreg[2], vreg[2], mreg;
  auto prefetch = [&](int t) {
    #pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int kg = t * KV + srow0 + 32 * half;
      if (kg < nk) {
        const int kph = axial ? ax_phys(kg, ax_t, ax_logS, ax_axis) : kg;
        kreg[half] = *reinterpret_cast<const int4v*>(kp + (long)kph * FA_D + sc8);
        vreg[half] = *reinterpret_cast<const int4v*>(vp + (long)kph * FA_D + sc8);
      } else {
        kreg[half] = int4v{0, 0, 0, 0};
        vreg[half] = int4v{0, 0, 0, 0};
      }
    }
    if (static_mask != nullptr) {
      const int mq = q0 + mrow;
      const int kb = t * KV;
      const long base = (long)mq * nk + kb + mc16;
      if (mq < nq && kb + mc16 + 16 <= nk && (base & 15) == 0) {
        mreg = *reinterpret_cast<const int4v*>(
            reinterpret_cast<const char*>(static_mask) + base);
      } else {
        unsigned char mb[16];
        #pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int kg = kb + mc16 + e;
          mb[e] = (mq < nq && kg < nk)
              ? (unsigned char)static_mask[(long)mq * nk + kg] : 0;
        }
        mreg = *reinterpret_cast<const int4v*>(mb);
      }
    }
  };

  int kt = next_live(0);
  if (kt < ntiles) prefetch(kt);

  while (kt < ntiles) {
    const int kbase = kt * KV;
    const int kt_next = next_live(kt + 1);

    __syncthreads();
    #pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int row = srow0 + 32 * half;
      *reinterpret_cast<int4v*>(&Kt[row][sc8]) = kreg[half];
      *reinterpret_cast<int4v*>(&Vr[row][sc8]) = vreg[half];
      const short* ks = reinterpret_cast<const short*>(&kreg[half]);
      #pragma unroll
      for (int e = 0; e < 8; ++e)
        Ktr[sc8 + e][swz_key(sc8 + e, row)] = ks[e];
    }
    if (static_mask != nullptr)
      *reinterpret_cast<int4v*>(&Mtile[mrow][mc16]) = mreg;
    __syncthreads();
    if (kt_next < ntiles) prefetch(kt_next);

    // s^T and dp^T, swapped layout: lane -> q = lq, keys = grp*4+r (+16mt)
    float s16[16], dp16[16];
    __builtin_amdgcn_s_setprio(1);
    #pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      f32x4 st{0, 0, 0, 0}, dpt{0, 0, 0, 0};
      #pragma unroll
      for (int c = 0; c < 2; ++c) {
        bf16x8 kf = frag_from_lds(&Kt[mt * 16 + lq][8 * grp + 32 * c]);
        bf16x8 vf = frag_from_lds(&Vr[mt * 16 + lq][8 * grp + 32 * c]);
        st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qfrag[c], st, 0, 0, 0);
        dpt = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, dofrag[c], dpt, 0, 0, 0);
      }
      #pragma unroll
      for (int r = 0; r < 4; ++r) { s16[mt * 4 + r] = st[r]; dp16[mt * 4 + r] = dpt[r]; }
    }
    __builtin_amdgcn_s_setprio(0);

    const bool interior = key_mask == nullptr &&
        (kbase + KV <= nk) && (q0 + FA_QBLK <= nq) &&
        (axial
             ? ((q0 >= ax_t && kbase + KV <= ax_t) ||
                (q0 + FA_QBLK <= ax_t && kbase + KV - 1 <= q0))
             : ((!causal || (kbase + KV - 1 <= q0 + diag)) &&
                (static_mask == nullptr ||
                 (tmap_row != nullptr && tmap_pair_full(tmap_row, kt, ntk)))));
    float ds16[16];
    if (interior) {
      #pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float p = fexp2(s16[i] * scl2 - lse_q);
        ds16[i] = p * (dp16[i] - D_q) * scale;
      }
    } else if (axial) {
      #pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int kg = kbase + (i >> 2) * 16 + grp * 4 + (i & 3);
        bool ok = (kg < nk) & (qrow < nq) & (kg <= qrow) &
                  ((kg < ax_t) | (kg >= ax_klo));
        if (key_mask != nullptr && ok)
          ok &= key_mask[(long)batch * nk + ax_phys(kg, ax_t, ax_logS, ax_axis)];
        const float p = ok ? fexp2(s16[i] * scl2 - lse_q) : 0.f;
        ds16[i] = p * (dp16[i] - D_q) * scale;
      }
    } else {
      #pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int kg = kbase + (i >> 2) * 16 + grp * 4 + (i & 3);
        bool ok = (kg < nk) & (qrow < nq);
        if (causal) ok &= kg <= qrow + diag;
        if (key_mask != nullptr && ok) ok &= key_mask[(long)batch * nk + kg];
        if (static_mask != nullptr && ok)
          ok &= Mtile[wave * 16 + lq][kg - kbase] != 0;
        const float p = ok ? fexp2(s16[i] * scl2 - lse_q) : 0.f;
        ds16[i] = p * (dp16[i] - D_q) * scale;
      }
    }
    #pragma unroll
    for (int a = 0; a < 4; ++a) {
      bf16x4 pk;
      #pragma unroll
      for (int e = 0; e < 4; ++e) pk[e] = f2bf(ds16[a * 4 + e]);
      *reinterpret_cast<bf16x4*>(&DSl[wave][lq][16 * a + 4 * grp]) = pk;
    }

    bf16x8 dsf0 = frag_from_lds(&DSl[wave][lq][8 * grp]);
    bf16x8 dsf1 = frag_from_lds(&DSl[wave][lq][32 + 8 * grp]);
    __builtin_amdgcn_s_setprio(1);
    #pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int d = lq + 16 * nt;
      bf16x8 kf0 = frag_from_lds(&Ktr[d][swz_key(d, 8 * grp)]);
      bf16x8 kf1 = frag_from_lds(&Ktr[d][swz_key(d, 32 + 8 * grp)]);
      acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsf0, kf0, acc[nt], 0, 0, 0);
      acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsf1, kf1, acc[nt], 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);

    kt = kt_next;
  }

  #pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qr = q0 + wave * 16 + grp * 4 + r;
    if (qr < nq) {
      const int qrp = axial ? ax_phys(qr, ax_t, ax_logS, ax_axis) : qr;
      #pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        dq[((long)bh * nq + qrp) * FA_D + 16 * nt + lq] = f2bf(acc[nt][r]);
      }
    }
  }
}

__global__ __launch_bounds__(256, 2)
void fa_bwd_dkv_kernel(
    const short* __restrict__ q,
    const short* __restrict__ k,
    const short* __restrict__ v,
    const short* __restrict__ dout,
    const float* __restrict__ lse,
    const float* __restrict__ Dv,
    short* __restrict__ dk,          // [bh, nk, 64]
    short* __restrict__ dv,          // [bh, nk, 64]
    const bool* __restrict__ key_mask,
    const bool* __restrict__ static_mask,
    const unsigned char* __restrict__ tile_map_t,  // [nk/64, nq/32]
    int b, int h, int nq, int nk, float scale, int causal, int do_bnhd,
    int ax_t, int ax_logS, int ax_axis) {

  constexpr int KV = 2 * FA_KBLK;          // 64 q rows per LDS tile
  __shared__ short Qr[KV][KPAD];           // Q rows (B-operand of s^T)
  __shared__ short dOr[KV][KPAD];          // dO rows (B-operand of dp^T)
  __shared__ short Qtr[FA_D][KV + 8];      // Q transposed (dK = dS^T Q)
  __shared__ short dOtr[FA_D][KV + 8];     // dO transposed (dV = P^T dO)
  __shared__ short Pt[FA_WAVES][16][KV + 8];
  __shared__ short DSt[FA_WAVES][16][KV + 8];
  __shared__ unsigned char Mtile[KV][FA_QBLK + 16];   // [q in tile][key in block] (80B stride)

  const int n_kt = (nk + FA_QBLK - 1) / FA_QBLK;
  int ktile, bh;
  xcd_chunked(blockIdx.x, n_kt * b * h, n_kt, &ktile, &bh);
  const int batch = bh / h;
  const int k0 = ktile * FA_QBLK;         // 64 keys per block
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int lq = lane & 15, grp = lane >> 4;
  const int krow = k0 + wave * 16 + lq;   // this lane's key (A-frag row)
  const int diag = nk - nq;

  const short* qp = q + (long)bh * nq * FA_D;
  const short* kp = k + (long)bh * nk * FA_D;
  const short* vp = v + (long)bh * nk * FA_D;
  const long do_stride = do_bnhd ? (long)h * FA_D : FA_D;
  const short* dop = do_bnhd
      ? dout + ((long)batch * nq * h + (bh - batch * h)) * FA_D
      : dout + (long)bh * nq * FA_D;

  const bool axial = ax_axis >= 0;
  const int kphys = axial ? ax_phys(krow, ax_t, ax_logS, ax_axis) : krow;
  // per accumulator row r: one past the last q row that may attend key
  // k0+wave*16+grp*4+r (text keys: everything causal; image keys: own line)
  int ax_kend[4];
  if (axial) {
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int key = k0 + wave * 16 + grp * 4 + r;
      ax_kend[r] = key < ax_t ? nq
          : min(nq, ax_t + ((((key - ax_t) >> ax_logS) + 1) << ax_logS));
    }
  }
  bf16x8 kfrag[2], vfrag[2];
  {
    const bool kok = krow < nk;
    #pragma unroll
    for (int c = 0; c < 2; ++c) {
      kfrag[c] = kok ? *reinterpret_cast<const bf16x8*>(kp + (long)kphys * FA_D + 8 * grp + 32 * c)
                     : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      vfrag[c] = kok ? *reinterpret_cast<const bf16x8*>(vp + (long)kphys * FA_D + 8 * grp + 32 * c)
                     : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }

  f32x4 acc_dk[4] = {f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0},
                     f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0}};
  f32x4 acc_dv[4] = {f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0},
                     f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0}};

  const int nqg = (nq + FA_KBLK - 1) / FA_KBLK;   // 32-row map granules
  const int nqt = (nq + KV - 1) / KV;             // 64-row compute tiles
  int qt_start = 0;
  if (causal) {
    const int qmin = k0 - diag;   // smallest q that sees any key here
    qt_start = qmin <= 0 ? 0 : qmin / KV;
  }
  __shared__ unsigned char TMrow[128];
  const unsigned char* tmap_row = stage_tmap_row(
      tile_map_t ? tile_map_t + (long)ktile * nqg : nullptr, nqg, TMrow);

  auto tile_live = [&](int t) -> bool {
    if (axial) {
      if (k0 < ax_t) return true;           // text keys: every causal q tile
      // image keys [k0, k0+64): queries live only inside the keys' lines
      const int lk1 = (min(k0 + FA_QBLK, nk) - 1 - ax_t) >> ax_logS;
      return t * KV < ax_t + ((lk1 + 1) << ax_logS);
    }
    return !tmap_row || tmap_pair_live(tmap_row, t, nqg);
  };
  auto next_live = [&](int t) -> int {
    while (t < nqt && !tile_live(t)) ++t;
    return t;
  };

  const int srow0 = tid >> 3;
  const int sc8 = (tid & 7) * 8;
  const int mrow = tid >> 2;
  const int mc16 = (tid & 3) * 16;
  int4v qreg[2], doreg[2], mreg;
  auto prefetch = [&](int t) {
    #pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int qg = t * KV + srow0 + 32 * half;
      if (qg < nq) {
        const int qph = axial ? ax_phys(qg, ax_t, ax_logS, ax_axis) : qg;
        qreg[half] = *reinterpret_cast<const int4v*>(qp + (long)qph * FA_D + sc8);
        doreg[half] = *reinterpret_cast<const int4v*>(dop + (long)qph * do_stride + sc8);
      } else {
        qreg[half] = int4v{0, 0, 0, 0};
        doreg[half] = int4v{0, 0, 0, 0};
      }
    }
    if (static_mask != nullptr) {
      const int mq = t * KV + mrow;            // q row of the streamed tile
      const long base = (long)mq * nk + k0 + mc16;
      if (mq < nq && k0 + mc16 + 16 <= nk && (base & 15) == 0) {
        mreg = *reinterpret_cast<const int4v*>(
            reinterpret_cast<const char*>(static_mask) + base);
      } else {
        unsigned char mb[16];
        #pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int kg = k0 + mc16 + e;
          mb[e] = (mq < nq && kg < nk)
              ? (unsigned char)static_mask[(long)mq * nk + kg] : 0;
        }
        mreg = *reinterpret_cast<const int4v*>(mb);
      }
    }
  };

  int qt = next_live(qt_start);
  if (qt < nqt) prefetch(qt);

  while (qt < nqt) {
    const int qbase = qt * KV;
    const int qt_next = next_live(qt + 1);

    __syncthreads();
    #pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int row = srow0 + 32 * half;
      *reinterpret_cast<int4v*>(&Qr[row][sc8]) = qreg[half];
      *reinterpret_cast<int4v*>(&dOr[row][sc8]) = doreg[half];
      const short* qs = reinterpret_cast<const short*>(&qreg[half]);
      const short* ds_ = reinterpret_cast<const short*>(&doreg[half]);
      #pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int kk = swz_key(sc8 + e, row);
        Qtr[sc8 + e][kk] = qs[e];
        dOtr[sc8 + e][kk] = ds_[e];
      }
    }
    if (static_mask != nullptr)
      *reinterpret_cast<int4v*>(&Mtile[mrow][mc16]) = mreg;
    __syncthreads();
    if (qt_next < nqt) prefetch(qt_next);

    // s^T[key, q], dp^T[key, q]: A = the wave's own key/value fragments,
    // B = Q/dO columns from LDS. Output [M=16 keys, N=16 q]: C row
    // grp*4+r = key within the wave's 16, C col = lane&15 = q in subtile.
    __builtin_amdgcn_s_setprio(1);
    const float scl2 = scale * 1.44269504088896f;
    f32x4 st4[4], dpt4[4];
    #pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      f32x4 st{0, 0, 0, 0}, dpt{0, 0, 0, 0};
      #pragma unroll
      for (int c = 0; c < 2; ++c) {
        bf16x8 qf = frag_from_lds(&Qr[mt * 16 + lq][8 * grp + 32 * c]);
        bf16x8 dof = frag_from_lds(&dOr[mt * 16 + lq][8 * grp + 32 * c]);
        st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfrag[c], qf, st, 0, 0, 0);
        dpt = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vfrag[c], dof, dpt, 0, 0, 0);
      }
      st4[mt] = st;
      dpt4[mt] = dpt;
    }
    __builtin_amdgcn_s_setprio(0);

    const bool interior = key_mask == nullptr &&
        (qbase + KV <= nq) && (k0 + FA_QBLK <= nk) &&
        (axial
             // text-key blocks under the causal bound; image-key blocks are
             // never interior (t=257 misaligns lines against 64-key blocks)
             ? (k0 + FA_QBLK <= ax_t && k0 + FA_QBLK - 1 <= qbase)
             : ((!causal || (k0 + FA_QBLK - 1 <= qbase + diag)) &&
                (static_mask == nullptr ||
                 (tmap_row != nullptr && tmap_pair_full(tmap_row, qt, nqg)))));
    if (interior) {
      #pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const int qg = qbase + mt * 16 + lq;
        const int qph = axial ? ax_phys(qg, ax_t, ax_logS, ax_axis) : qg;
        const float l = lse[(long)bh * nq + qph] * 1.44269504088896f;
        const float Dq = Dv[(long)bh * nq + qph];
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = fexp2(st4[mt][r] * scl2 - l);
          const float ds = p * (dpt4[mt][r] - Dq) * scale;
          const int cc = (mt * 16 + lq) ^ (grp << 3);   // swz by row>>2
          Pt[wave][grp * 4 + r][cc] = f2bf(p);
          DSt[wave][grp * 4 + r][cc] = f2bf(ds);
        }
      }
    } else if (axial) {
      #pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const int qg = qbase + mt * 16 + lq;
        const int qph = (qg < nq) ? ax_phys(qg, ax_t, ax_logS, ax_axis) : 0;
        const float l = (qg < nq)
            ? lse[(long)bh * nq + qph] * 1.44269504088896f : 0.f;
        const float Dq = (qg < nq) ? Dv[(long)bh * nq + qph] : 0.f;
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = k0 + wave * 16 + grp * 4 + r;
          bool ok = (key < nk) & (qg < nq) & (qg >= key) & (qg < ax_kend[r]);
          if (key_mask != nullptr && ok)
            ok &= key_mask[(long)batch * nk + ax_phys(key, ax_t, ax_logS, ax_axis)];
          float p = 0.f, ds = 0.f;
          if (ok) {
            p = fexp2(st4[mt][r] * scl2 - l);
            ds = p * (dpt4[mt][r] - Dq) * scale;
          }
          const int cc = (mt * 16 + lq) ^ (grp << 3);
          Pt[wave][grp * 4 + r][cc] = f2bf(p);
          DSt[wave][grp * 4 + r][cc] = f2bf(ds);
        }
      }
    } else {
      #pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = k0 + wave * 16 + grp * 4 + r;
          const int qg = qbase + mt * 16 + lq;
          bool ok = (key < nk) & (qg < nq);
          if (causal) ok &= key <= qg + diag;
          if (key_mask != nullptr && ok) ok &= key_mask[(long)batch * nk + key];
          if (static_mask != nullptr && ok)
            ok &= Mtile[mt * 16 + lq][key - k0] != 0;
          float p = 0.f, ds = 0.f;
          if (ok) {
            const float l = lse[(long)bh * nq + qg] * 1.44269504088896f;
            const float Dq = Dv[(long)bh * nq + qg];
            p = fexp2(st4[mt][r] * scl2 - l);
            ds = p * (dpt4[mt][r] - Dq) * scale;
          }
          const int cc = (mt * 16 + lq) ^ (grp << 3);   // swz by row>>2
          Pt[wave][grp * 4 + r][cc] = f2bf(p);
          DSt[wave][grp * 4 + r][cc] = f2bf(ds);
        }
      }
    }

    const int rsw = ((lq >> 2) & 7) << 3;               // same swz, row = lq
    bf16x8 pf0 = frag_from_lds(&Pt[wave][lq][(8 * grp) ^ rsw]);
    bf16x8 pf1 = frag_from_lds(&Pt[wave][lq][(32 + 8 * grp) ^ rsw]);
    bf16x8 dsf0 = frag_from_lds(&DSt[wave][lq][(8 * grp) ^ rsw]);
    bf16x8 dsf1 = frag_from_lds(&DSt[wave][lq][(32 + 8 * grp) ^ rsw]);
    __builtin_amdgcn_s_setprio(1);
    #pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int d = lq + 16 * nt;
      bf16x8 dof0 = frag_from_lds(&dOtr[d][swz_key(d, 8 * grp)]);
      bf16x8 dof1 = frag_from_lds(&dOtr[d][swz_key(d, 32 + 8 * grp)]);
      bf16x8 qf0 = frag_from_lds(&Qtr[d][swz_key(d, 8 * grp)]);
      bf16x8 qf1 = frag_from_lds(&Qtr[d][swz_key(d, 32 + 8 * grp)]);
      acc_dv[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf0, dof0, acc_dv[nt], 0, 0, 0);
      acc_dv[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf1, dof1, acc_dv[nt], 0, 0, 0);
      acc_dk[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsf0, qf0, acc_dk[nt], 0, 0, 0);
      acc_dk[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsf1, qf1, acc_dk[nt], 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);

    qt = qt_next;
  }

  #pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int kr = k0 + wave * 16 + grp * 4 + r;
    if (kr < nk) {
      const int krp = axial ? ax_phys(kr, ax_t, ax_logS, ax_axis) : kr;
      #pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        dk[((long)bh * nk + krp) * FA_D + 16 * nt + lq] = f2bf(acc_dk[nt][r]);
        dv[((long)bh * nk + krp) * FA_D + 16 * nt + lq] = f2bf(acc_dv[nt][r]);
      }
    }
  }
}

// D = rowsum(dO * O) for the flash backward, fused (the ATen form costs
// two full fp32 materializations of dO and O per attention backward).
// 4 lanes per row, 32B vector loads, shfl reduce.
__global__ void fa_dv_kernel(
    const short* __restrict__ dout, const short* __restrict__ out,
    float* __restrict__ Dv, int b, int h, int nq, int do_bnhd) {
  const int bh = blockIdx.y;
  const int batch = bh / h;
  const long stride = do_bnhd ? (long)h * 64 : 64;
  const long base = do_bnhd
      ? ((long)batch * nq * h + (bh - batch * h)) * 64
      : (long)bh * nq * 64;
  const int row = blockIdx.x * 64 + (threadIdx.x >> 2);
  const int part = (threadIdx.x & 3) * 16;
  if (row >= nq) return;
  const short* dp = dout + base + row * stride + part;
  const short* op = out + base + row * stride + part;
  float acc = 0.f;
  #pragma unroll
  for (int c = 0; c < 2; ++c) {
    int4v dv16 = *reinterpret_cast<const int4v*>(dp + 8 * c);
    int4v ov16 = *reinterpret_cast<const int4v*>(op + 8 * c);
    const short* ds_ = reinterpret_cast<const short*>(&dv16);
    const short* os_ = reinterpret_cast<const short*>(&ov16);
    #pragma unroll
    for (int e = 0; e < 8; ++e) acc += bf2f(ds_[e]) * bf2f(os_[e]);
  }
  acc += __shfl_xor(acc, 1);
  acc += __shfl_xor(acc, 2);
  if ((threadIdx.x & 3) == 0) Dv[(long)bh * nq + row] = acc;
}

// ---------------------------------------------------------------------------
// MFMA layout probe (test support): one 16x16x32 bf16 MFMA with the exact
// fragment mappings the attention kernel assumes. The GPU test compares
// C against torch.matmul on asymmetric inputs (guide G9) so a wrong operand
// layout is caught in isolation.
// ---------------------------------------------------------------------------

__global__ void mfma_probe_kernel(const short* __restrict__ A,   // [16,32]
                                  const short* __restrict__ B,   // [32,16]
                                  float* __restrict__ C) {       // [16,16]
  const int lane = threadIdx.x & 63;
  const int lq = lane & 15, grp = lane >> 4;
  bf16x8 af = *reinterpret_cast<const bf16x8*>(A + lq * 32 + 8 * grp);
  bf16x8 bf;
  #pragma unroll
  for (int e = 0; e < 8; ++e) bf[e] = B[(8 * grp + e) * 16 + lq];
  f32x4 c{0, 0, 0, 0};
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, c, 0, 0, 0);
  #pragma unroll
  for (int r = 0; r < 4; ++r) C[(grp * 4 + r) * 16 + lq] = c[r];
}

// ===========================================================================
// Host wrappers
// ===========================================================================

static int ax_log2(int64_t S) {
  int logS = 0;
  while ((1 << logS) < S) ++logS;
  TORCH_CHECK((1 << logS) == S, "axial image_size must be a power of 2");
  return logS;
}

TensorList fa_fwd(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                  double scale, bool causal, OptTensor key_mask,
                  OptTensor static_mask, OptTensor tile_map, bool out_bnhd,
                  int64_t ax_t, int64_t ax_S, int64_t ax_axis) {
  CHK(q.is_cuda() && k.is_cuda() && v.is_cuda());
  CHK(q.dtype() == torch::kBFloat16);
  CHK(q.size(-1) == FA_D);
  CHK(q.is_contiguous() && k.is_contiguous() && v.is_contiguous());
  const int b = q.size(0), h = q.size(1), nq = q.size(2), nk = k.size(2);
  const int ax_logS = ax_axis >= 0 ? ax_log2(ax_S) : 0;
  if (ax_axis >= 0) {
    CHK(causal && nq == nk && !static_mask.has_value() && !tile_map.has_value());
  }

  auto out = out_bnhd ? torch::empty({b, nq, h, FA_D}, q.options())
                      : torch::empty_like(q);
  auto lse = torch::empty({b, h, nq}, q.options().dtype(torch::kFloat32));

  const bool* km = nullptr;
  const bool* sm = nullptr;
  const unsigned char* tm = nullptr;
  if (key_mask.has_value()) {
    CHK(key_mask->dtype() == torch::kBool && key_mask->is_contiguous());
    CHK(key_mask->size(0) == b && key_mask->size(1) == nk);
    km = key_mask->data_ptr<bool>();
  }
  if (static_mask.has_value()) {
    CHK(static_mask->dtype() == torch::kBool && static_mask->is_contiguous());
    CHK(static_mask->size(0) == nq && static_mask->size(1) == nk);
    sm = static_mask->data_ptr<bool>();
  }
  if (tile_map.has_value()) {
    CHK(tile_map->dtype() == torch::kUInt8 && tile_map->is_contiguous());
    CHK(tile_map->size(0) == (nq + FA_QBLK - 1) / FA_QBLK);
    CHK(tile_map->size(1) == (nk + FA_KBLK - 1) / FA_KBLK);
    tm = tile_map->data_ptr<uint8_t>();
  }

  // 8-wave 32x32 ladder (DALLE_AMD_FA8=1 opt-in). Measured on MI355X at the
  // flagship shape it LOSES to the 4-wave 16x16 kernel (dense 819 vs 722 us,
  // axial 835 vs 502): at D=64 the ladder has half the MFMA work per softmax
  // op of the guide's D=128 recipe and PMC shows it VALU-bound (42 VALU
  // instrs per MFMA), while its 256-row blocks waste 7/8 of the staged grid
  // lines under axial patterns. Kept correct + tested for D=128-class heads.
  const char* fa8_env = getenv("DALLE_AMD_FA8");
  const bool fa8_on = fa8_env != nullptr && fa8_env[0] == '1';
  if (fa8_on && sm == nullptr && tm == nullptr && nq >= 64) {
    dim3 grid8(((nq + FA8_QBLK - 1) / FA8_QBLK) * b * h);
    hipLaunchKernelGGL(fa8_fwd_d64_kernel, grid8, dim3(512), 0, cur_stream(),
                       bf16_cptr(q), bf16_cptr(k), bf16_cptr(v), bf16_ptr(out),
                       lse.data_ptr<float>(), km, b, h, nq, nk, (float)scale,
                       causal ? 1 : 0, out_bnhd ? 1 : 0, (int)ax_t, ax_logS,
                       (int)ax_axis);
    return {out, lse};
  }
  dim3 grid(((nq + FA_QBLK - 1) / FA_QBLK) * b * h);
  hipLaunchKernelGGL(fa_fwd_d64_kernel, grid, dim3(256), 0, cur_stream(),
                     bf16_cptr(q), bf16_cptr(k), bf16_cptr(v), bf16_ptr(out),
                     lse.data_ptr<float>(), km, sm, tm, b, h, nq, nk,
                     (float)scale, causal ? 1 : 0, out_bnhd ? 1 : 0, (int)ax_t,
                     ax_logS, (int)ax_axis);
  return {out, lse};
}

TensorList permlane_probe(torch::Tensor a, torch::Tensor b_) {
  CHK(a.is_cuda() && a.dtype() == torch::kInt32 && a.numel() == 64);
  auto r0 = torch::empty_like(a);
  auto r1 = torch::empty_like(a);
  hipLaunchKernelGGL(permlane_probe_kernel, dim3(1), dim3(64), 0, cur_stream(),
                     reinterpret_cast<const unsigned*>(a.data_ptr()),
                     reinterpret_cast<const unsigned*>(b_.data_ptr()),
                     reinterpret_cast<unsigned*>(r0.data_ptr()),
                     reinterpret_cast<unsigned*>(r1.data_ptr()));
  return {r0, r1};
}

TensorList fa_bwd(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                  torch::Tensor out, torch::Tensor lse, torch::Tensor dout,
                  double scale, bool causal, OptTensor key_mask,
                  OptTensor static_mask, OptTensor tile_map,
                  OptTensor tile_map_t, bool out_bnhd, OptTensor grad_lse,
                  int64_t ax_t, int64_t ax_S, int64_t ax_axis) {
  CHK(q.is_cuda() && q.dtype() == torch::kBFloat16);
  CHK(q.is_contiguous() && k.is_contiguous() && v.is_contiguous());
  CHK(out.is_contiguous() && dout.is_contiguous());
  const int b = q.size(0), h = q.size(1), nq = q.size(2), nk = k.size(2);
  const int ax_logS = ax_axis >= 0 ? ax_log2(ax_S) : 0;

  auto Dv = torch::empty({b, h, nq}, q.options().dtype(torch::kFloat32));
  {
    dim3 grid_d((nq + 63) / 64, b * h);
    hipLaunchKernelGGL(fa_dv_kernel, grid_d, dim3(256), 0, cur_stream(),
                       bf16_cptr(dout), bf16_cptr(out), Dv.data_ptr<float>(),
                       b, h, nq, out_bnhd ? 1 : 0);
  }
  if (grad_lse.has_value()) {
    // dL/dS_j = P_j * (dP_j - (D - g_lse)): an upstream logsumexp gradient
    // (the axial lse-merge path) folds into the per-row delta term
    CHK(grad_lse->dtype() == torch::kFloat32);
    CHK(grad_lse->sizes() == Dv.sizes());
    Dv.sub_(*grad_lse);
  }

  auto dq = torch::empty_like(q);
  auto dk = torch::empty_like(k);
  auto dv = torch::empty_like(v);

  const bool* km = nullptr;
  const bool* sm = nullptr;
  const unsigned char* tm = nullptr;
  const unsigned char* tmt = nullptr;
  if (key_mask.has_value()) km = key_mask->data_ptr<bool>();
  if (static_mask.has_value()) sm = static_mask->data_ptr<bool>();
  if (tile_map.has_value()) tm = tile_map->data_ptr<uint8_t>();
  if (tile_map_t.has_value()) tmt = tile_map_t->data_ptr<uint8_t>();

  dim3 grid_q(((nq + FA_QBLK - 1) / FA_QBLK) * b * h);
  hipLaunchKernelGGL(fa_bwd_dq_kernel, grid_q, dim3(256), 0, cur_stream(),
                     bf16_cptr(q), bf16_cptr(k), bf16_cptr(v), bf16_cptr(dout),
                     lse.data_ptr<float>(), Dv.data_ptr<float>(), bf16_ptr(dq),
                     km, sm, tm, b, h, nq, nk, (float)scale, causal ? 1 : 0,
                     out_bnhd ? 1 : 0, (int)ax_t, ax_logS, (int)ax_axis);
  dim3 grid_k(((nk + FA_QBLK - 1) / FA_QBLK) * b * h);
  hipLaunchKernelGGL(fa_bwd_dkv_kernel, grid_k, dim3(256), 0, cur_stream(),
                     bf16_cptr(q), bf16_cptr(k), bf16_cptr(v), bf16_cptr(dout),
                     lse.data_ptr<float>(), Dv.data_ptr<float>(), bf16_ptr(dk),
                     bf16_ptr(dv), km, sm, tmt, b, h, nq, nk, (float)scale,
                     causal ? 1 : 0, out_bnhd ? 1 : 0, (int)ax_t, ax_logS,
                     (int)ax_axis);
  return {dq, dk, dv};
}

torch::Tensor mfma_probe(torch::Tensor A, torch::Tensor B) {
  CHK(A.is_cuda() && A.dtype() == torch::kBFloat16);
  auto Ac = A.contiguous();
  auto Bc = B.contiguous();
  auto C = torch::zeros({16, 16}, A.options().dtype(torch::kFloat32));
  hipLaunchKernelGGL(mfma_probe_kernel, dim3(1), dim3(64), 0, cur_stream(),
                     bf16_cptr(Ac), bf16_cptr(Bc), C.data_ptr<float>());
  return C;
}
