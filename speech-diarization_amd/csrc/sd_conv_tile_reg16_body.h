// The body of the two register-staged 128x128 kernels of sd_conv_gemm_f16.hip, conv_gemm_f16_kernel<TA, TO> and
// conv_gemm_split16_n128_kernel<TO>: one 128x128 output tile, both operands staged through registers.  Included INSIDE each kernel,
// which provides
//   P         the policy (RegF16<TA> / RegSplit16, defined beside the kernels): activation type, what a thread holds of an activation
//             row, values per K step, whether the activations are split into f16 halves on their way into LDS
//   TO        the output type
//   p, vec    the kernel's arguments, and smem_raw, its dynamic LDS
// Text and not a __device__ function: called as a function (arguments by reference or by value, LDS passed in or declared inside)
// every instantiation of both kernels comes out with 60-86 changed lines of scalar code, and the rule of DESIGN.md section 12 is
// that a shared statement leaves the device code as it was (tools/isa_diff.py).  No include guard: it is included twice.
  using TX = typename P::TA;                              // the activations' type in memory
  _Float16* As = reinterpret_cast<_Float16*>(smem_raw);  // [2][BM][LDP]
  _Float16* Bs = As + 2 * BM * LDP;                       // [2][BN][LDP]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;

  // XCD-aware, bijective remap: consecutive tiles (n fastest: they share the A row panel) go
  // to one XCD instead of being dealt round-robin over the eight L2s
  const int n_tiles = (p.cout + BN - 1) / BN;
  const int wg = sd_xcd_tile(blockIdx.x, gridDim.x);
  const int tile_n = wg % n_tiles;
  const int tile_m = wg / n_tiles;
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  // staging role: 8 threads per row, 4 rows per thread; all loads unconditional (rows/channels past the end clamp to the last
  // valid one and are never stored, columns past cin re-read column 0 against the zero-filled weight padding).  A: thread c8 owns
  // values AV c8 .. AV c8 + AV - 1 of the step's KV (16 bytes of f16, 16 or 32 bytes of f32); B: halfs 8 c8 .. 8 c8 + 7 of the 64
  // (one 16-byte load of the packed weights)
  const int c8 = tid & 7;
  const int r0 = tid >> 3;
  int a_seg[4], a_t[4];
  const _Float16* wptr[4];
  const TX* aptr[4];
  const int ktot = p.taps * p.cin_pad;                    // values per output channel (SPLIT: 2 halfs each)
  const _Float16* W = static_cast<const _Float16*>(p.w);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int m = m0 + r0 + 32 * i;
    m = m < p.M ? m : p.M - 1;
    const int seg = (m / p.T) * p.T;
    a_seg[i] = seg;
    a_t[i] = m - seg;
    int n = n0 + r0 + 32 * i;
    n = n < p.cout ? n : p.cout - 1;
    if constexpr (P::SPLIT) wptr[i] = W + (size_t)n * 2 * ktot + c8 * 8;
    else wptr[i] = W + (size_t)n * ktot + c8 * 8;
  }
  const int nk = p.taps * (p.cin_pad / P::KV);
  const int half = p.taps / 2;
  const TX* X = static_cast<const TX*>(p.x) + p.a_col0;

  auto set_tap = [&](int tap) {
    const int delta = (tap - half) * p.dil;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int tt = a_t[i] + delta;
      tt = sd_reflect(tt, p.T);
      aptr[i] = X + (size_t)(a_seg[i] + tt) * p.lda;
    }
  };

  // Two register stages: the fetch runs TWO K steps ahead of the MFMAs (one step is only ~0.2 us of
  // matrix work, far less than an HBM/L2 round trip), the LDS stage one step ahead.
  struct Stage { typename P::AVec a[4]; h8 b[4]; };
  Stage s0, s1;
  int ld_tap = 0, ld_c0 = 0;
  set_tap(0);
  auto gload = [&](Stage& st) {
    const int col = ld_c0 + c8 * P::AV;
    const int acol = col < p.cin ? col : 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      st.a[i] = P::load_a(aptr[i] + acol);
      st.b[i] = *reinterpret_cast<const h8*>(wptr[i]);
      wptr[i] += BK;
    }
    ld_c0 += P::KV;
    if (ld_c0 >= p.cin_pad) {
      ld_c0 = 0;
      ++ld_tap;
      if (ld_tap < p.taps) set_tap(ld_tap);
    }
  };
  auto lstore = [&](const Stage& st, int buf) {
    _Float16* a = As + buf * BM * LDP;
    _Float16* b = Bs + buf * BN * LDP;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (P::SPLIT) {
        h4 hi, lo;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float w = sd_split16_clamp(st.a[i][e]);
          hi[e] = (_Float16)w;
          lo[e] = (_Float16)(w - (float)hi[e]);
        }
        *reinterpret_cast<h4*>(a + (r0 + 32 * i) * LDP + c8 * 4) = hi;
        *reinterpret_cast<h4*>(a + (r0 + 32 * i) * LDP + 32 + c8 * 4) = lo;
      } else {
        *reinterpret_cast<h8*>(a + (r0 + 32 * i) * LDP + c8 * 8) = st.a[i];
      }
      *reinterpret_cast<h8*>(b + (r0 + 32 * i) * LDP + c8 * 8) = st.b[i];
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int frag_row = lane & 31;
  const int frag_k = (lane >> 5) * 8;

  struct Frag { h8 a0, a1, b0, b1; };
  auto fread = [&](const _Float16* a, const _Float16* b, int kk) {
    Frag f;
    f.a0 = *reinterpret_cast<const h8*>(a + kk * 16);
    f.a1 = *reinterpret_cast<const h8*>(a + 32 * LDP + kk * 16);
    f.b0 = *reinterpret_cast<const h8*>(b + kk * 16);
    f.b1 = *reinterpret_cast<const h8*>(b + 32 * LDP + kk * 16);
    return f;
  };
  auto mma = [&](const Frag& fa, const Frag& fb) {        // A fragments of fa against B fragments of fb
    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa.a0, fb.b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa.a0, fb.b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa.a1, fb.b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa.a1, fb.b1, acc[1][1], 0, 0, 0);
  };

  gload(s0);                 // K step 0
  if (nk > 1) gload(s1);     // K step 1
  lstore(s0, 0);
  if (nk > 2) gload(s0);     // K step 2
  __syncthreads();

  int cur = 0;
  // one K step: MFMAs on LDS stage `cur`; `st` holds step kt+1 -> written to the other LDS stage,
  // then refilled with step kt+3
  auto kstep = [&](int kt, Stage& st) {
    const _Float16* a = As + cur * BM * LDP + (wm * 64 + frag_row) * LDP + frag_k;
    const _Float16* b = Bs + cur * BN * LDP + (wn * 64 + frag_row) * LDP + frag_k;
    if constexpr (P::SPLIT) {
      // the four 16-half fragment slices hi0, hi1, lo0, lo1 and six MFMA groups, hi.hi + hi.lo + lo.hi per value slice
      const Frag h0 = fread(a, b, 0);           // hi, values 0-15
      const Frag l0 = fread(a, b, 2);           // lo, values 0-15
      mma(h0, h0);
      const Frag h1 = fread(a, b, 1);           // hi, values 16-31
      mma(h0, l0);
      mma(l0, h0);
      const Frag l1 = fread(a, b, 3);           // lo, values 16-31
      if (kt + 1 < nk) lstore(st, cur ^ 1);
      if (kt + 3 < nk) gload(st);
      mma(h1, h1);
      mma(h1, l1);
      mma(l1, h1);
    } else {
      Frag f0 = fread(a, b, 0);
      Frag f1 = fread(a, b, 1);
      mma(f0, f0);
      f0 = fread(a, b, 2);
      mma(f1, f1);
      f1 = fread(a, b, 3);
      if (kt + 1 < nk) lstore(st, cur ^ 1);
      if (kt + 3 < nk) gload(st);
      mma(f0, f0);
      mma(f1, f1);
    }
    __syncthreads();
    cur ^= 1;
  };
  for (int kt = 0; kt < nk; kt += 2) {
    kstep(kt, s1);
    if (kt + 1 < nk) kstep(kt + 1, s0);
  }

  // ---- epilogue: raw accumulators (SPLIT: x 2^-s, exact: the weights carry a power-of-two scale 2^s that keeps their low halves out
  // of the f16 subnormals) -> LDS C tile -> sd_store_tile (sd_epilogue.h)
  float* Cs = reinterpret_cast<float*>(smem_raw);
  if constexpr (P::SPLIT) {
    const float alpha = p.w_scale_inv != 0.f ? p.w_scale_inv : 1.f;
    SD_ACC32_TO_TILE(Cs, LDC, wm * 64, wn * 64, 2, 2, lane, acc[mi][ni][r] * alpha);
  } else {
    SD_ACC32_TO_TILE(Cs, LDC, wm * 64, wn * 64, 2, 2, lane, acc[mi][ni][r]);
  }
  __syncthreads();
  sd_store_tile<TO, BM, BN, 256, 2, 3, P::SPLIT>(p, Cs, LDC, m0, n0, tid, vec);      // (SPLIT: the only kernel that may write y as SD_DT_SPLIT16)
