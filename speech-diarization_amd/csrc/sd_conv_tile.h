// The rules the matrix-core kernels of sd_conv_gemm.hip, sd_conv_gemm_f16.hip, sd_affinity.hip, sd_fbank*.hip and sd_res2net_f16.hip
// share, each stated once: device-side helpers, and at the end the host side of a conv launch.  Every __global__ kernel and every launch
// label stays in its .hip file.
//
// A helper replaces a kernel's own text only where the compiler emits the same device code as before (tools/isa_diff.py against the
// parent commit).  Where it does not, the kernel keeps its own text behind a comment that names the helper.
#pragma once
#include "sd_common.h"

// 16 bytes per lane from global memory straight into LDS (global_load_lds_dwordx4): no VGPR staging.  The LDS side of a wave's
// instruction is lane-linear (64 x 16 bytes from lptr, which is wave-uniform); the global side is per lane.
#define SD_GLDS16(gptr, lptr)                                                              \
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gptr),  \
                                   (__attribute__((address_space(3))) void*)(lptr), 16, 0, 0)

// Reflect padding: index t of a row of T, |overhang| < T, mirrored at both ends without repeating the edge (-1 -> 1, T -> T - 2)
__device__ __forceinline__ int sd_reflect(int t, int T) {
  t = t < 0 ? -t : t;
  return t >= T ? 2 * (T - 1) - t : t;
}

// XCD remap.  The hardware deals workgroups round-robin over the eight XCDs (one L2 each): workgroup b runs on XCD b % 8, as that
// XCD's workgroup number b / 8.  Of a list of n entries the XCD of workgroup b owns the contiguous range [sd_xcd_first, + sd_xcd_count)
// (the first n % 8 XCDs hold one more), so neighbours in the list, which share an operand panel, meet in one L2.  sd_xcd_tile: the
// entry of workgroup b in a launch of nwg workgroups, one per entry (a bijection of [0, nwg)).
__device__ __forceinline__ int sd_xcd_first(int b, int n) {
  const int q = n >> 3, r = n & 7, xcd = b & 7;
  return xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
}
__device__ __forceinline__ int sd_xcd_count(int b, int n) { return (n >> 3) + ((b & 7) < (n & 7) ? 1 : 0); }
__device__ __forceinline__ int sd_xcd_tile(int b, int nwg) { return sd_xcd_first(b, nwg) + (b >> 3); }

// a <-> b on one lane bit (v_permlane16_swap / v_permlane32_swap), for any 32-bit T: the odd 16-lane rows of a trade with the even
// rows of b / the upper 32 lanes of a with the lower 32 of b
template <typename T>
__device__ __forceinline__ void sd_swap16(T& a, T& b) {
  static_assert(sizeof(T) == 4, "one register per lane");
  const auto w = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b), false, false);
  const unsigned w0 = w[0], w1 = w[1];       // (a bit_cast applied to the vector ELEMENT reads element 0 for both: hipcc 7.2)
  a = __builtin_bit_cast(T, w0);
  b = __builtin_bit_cast(T, w1);
}
template <typename T>
__device__ __forceinline__ void sd_swap32(T& a, T& b) {
  static_assert(sizeof(T) == 4, "one register per lane");
  const auto w = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b), false, false);
  const unsigned w0 = w[0], w1 = w[1];
  a = __builtin_bit_cast(T, w0);
  b = __builtin_bit_cast(T, w1);
}

// Accumulator layout of the 32x32 MFMAs: register r of lane l holds C[(r & 3) + 8 (r >> 2) + 4 (l >> 5)][l & 31].  MI x NI accumulators
// of one wave, tile (mi, ni) at (row0 + 32 mi, col0 + 32 ni), into the epilogue's C tile Cs in LDS (row stride ldc floats).  `value` is an
// expression in mi, ni and r: acc[mi][ni][r], acc[r], acc[mi][ni][r] * alpha.  (A macro, like the kernels' own fragment macros: as a
// function that takes the accumulators by reference it changes the register allocation of every kernel it was tried in.)
#define SD_ACC32_TO_TILE(Cs_, ldc_, row0_, col0_, MI_, NI_, lane_, value)                    \
  do {                                                                                       \
    const int hrow_ = ((lane_) >> 5) * 4;                                                    \
    _Pragma("unroll") for (int ni = 0; ni < (NI_); ++ni) {                                   \
      const int cl_ = (col0_) + ni * 32 + ((lane_) & 31);                                    \
      _Pragma("unroll") for (int mi = 0; mi < (MI_); ++mi) {                                 \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                     \
          const int rl_ = (row0_) + mi * 32 + (r & 3) + 8 * (r >> 2) + hrow_;                \
          (Cs_)[rl_ * (ldc_) + cl_] = (value);                                               \
        }                                                                                    \
      }                                                                                      \
    }                                                                                        \
  } while (0)

// ---- host side of the conv launches

// the algorithmic flops of a conv launch (SdProfScope's work figure)
static inline double sd_conv_flops(const sd_conv_args* a) { return 2.0 * (double)a->M * (double)a->cout * (double)a->taps * (double)a->cin; }

// sd_func_max_lds + SdProfScope + hipLaunchKernelGGL of one conv kernel; the caller follows it with SD_CHECK_LAUNCH("<label>"), where the
// label stays a string literal chosen by the expression that picked `kern`.  prof_kind < 0: a launch outside the per-kernel timing (work unused);
// lds = 0: no dynamic LDS to allow.  Returns what sd_func_max_lds returned (launch errors are SD_CHECK_LAUNCH's to read).
template <typename... P, typename... A>
static inline hipError_t sd_launch_conv(void (*kern)(P...), int prof_kind, double work, long grid, int block, size_t lds, hipStream_t stream,
                                        A... args) {
  if (lds) {
    const hipError_t e = sd_func_max_lds(reinterpret_cast<const void*>(kern), (int)lds);
    if (e != hipSuccess) return e;
  }
  if (prof_kind >= 0) {
    SdProfScope prof(prof_kind, stream, work);
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(block), lds, stream, args...);
  } else {
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(block), lds, stream, args...);
  }
  return hipSuccess;
}
