// Which kernel a conv operator launches, and with what grid: the CHOICE, pure and host-only.
//
// Every operator of sd_conv_gemm.hip / sd_conv_gemm_f16.hip is check (sd_check_conv), choose (a function of this header), launch (one
// switch over SdConvChoice::kernel).  A choice is a function of the shape fields of sd_conv_args, of `vec` (what sd_check_conv made of
// the alignments), of the caller's flags and of one SdConvTuning snapshot -- and of nothing else: no pointer's value beyond null / not
// null, no environment variable, no device query, no atomic, no launch.  This header includes no HIP header, so the same functions
// compile into a plain C++ program (tests/test_conv_choice_rules.py) and serve sd_conv_choice_read (sd_hip_trace.h).
// Each condition stands here once, as a named predicate with the measurement it rests on; sd_ecapa.hip's plan and SdConvRule use the
// same ones.
#pragma once
#include <stddef.h>

#include "sd_hip.h"

// ---------------------------------------------------------------- tuning: one snapshot per call (per ECAPA forward)
// tune[key]: the value of sd_set_tuning(key, .), index 0 unused.  n_cu: the device's CU count (0: unknown).  The two experiment
// switches are read behind sd_experiment_env by sd_conv_tuning_now (sd_conv_gemm.hip), once per process.
struct SdConvTuning {
  long tune[SD_TUNE_T256_LOCKSTEP_TILES + 1];
  int n_cu;
  int f16_kernel;        // SD_F16_KERNEL=reg|t256 (tools/stamp_t256.py, A/B runs): 0 / 2 force that kernel, -1 by the rule
  bool t256_direct;      // SD_T256_DIRECT=0 (A/B runs): the LDS-staged epilogue for every layer
};

// What sd_set_tuning(key, negative) restores.
constexpr long sd_tune_default(int key) {
  switch (key) {
    case SD_TUNE_SKINNY_TILES: return 128L;          // measured at 16 / 32 / 64 / 128 segments: 128 beats 256 and 512
    case SD_TUNE_WIDE_TILES: return 1024L;           // at least four rounds of 256x256 tiles over the CUs
    case SD_TUNE_F16_NARROW_TILES: return 128L;      // sd_wide_goes_narrow
    // measured (tools/probe_small_shapes.py): Res2Net conv at 64 segments (101 tiles of 128x128) 19 us against 31 on the 128x128 kernel,
    // at 128 segments (201 tiles) 37 against 34
    case SD_TUNE_S64_TILES: return 128L;
    default: return -1L;                             // HALF_TILES, TILE_ROWS: by the cost rule; T256_LOCKSTEP_TILES: 4 x 256 tiles
  }
}
// The value sd_set_tuning stores for (key, value).  HALF_TILES: 0 never, 1 whenever possible.  TILE_ROWS: 0 128-row tiles only, 80 / 96 /
// 112 that height whenever possible.
constexpr long sd_tune_stored(int key, long value) {
  return value < 0 ? sd_tune_default(key) : key == SD_TUNE_HALF_TILES ? (value ? 1L : 0L) : value;
}
inline SdConvTuning sd_conv_tuning_default(int n_cu) {
  SdConvTuning t = {};
  for (int k = 1; k <= SD_TUNE_T256_LOCKSTEP_TILES; ++k) t.tune[k] = sd_tune_default(k);
  t.n_cu = n_cu; t.f16_kernel = -1; t.t256_direct = true;
  return t;
}
SdConvTuning sd_conv_tuning_now(int n_cu = -1);     // sd_conv_gemm.hip: the stored values; n_cu < 0: the current device's, asked once per process

// ---------------------------------------------------------------- the choice
enum SdConvKernel {
  SD_K_F32_S64_32, SD_K_F32_S64_64, SD_K_F32_SKINNY, SD_K_F32_T256, SD_K_F32_VH5, SD_K_F32_VH6, SD_K_F32_VH7, SD_K_F32_N64, SD_K_F32_128,
  SD_K_F32_128_SYMMETRIC, SD_K_F32_PACKED, SD_K_SEG_PARTIAL, SD_K_SEG_REDUCE,
  SD_K_F16_128_HH, SD_K_F16_128_HF, SD_K_F16_128_FH, SD_K_F16_128_FF,          // <x, y>: H f16, F f32
  SD_K_F16_T256_H_DIRECT, SD_K_F16_T256_H_STAGED, SD_K_F16_T256_F_DIRECT, SD_K_F16_T256_F_STAGED,      // <y, epilogue>
  SD_K_SPLIT_T256_DIRECT, SD_K_SPLIT_T256_STAGED, SD_K_SPLIT_N128
};

// The launch label of a kernel id (sd_common.h SD_CHECK_LAUNCH, the census of tests/helpers/kernel_census.py): the kernel's name, <...>
// for the instantiation, /... for the walk.  Literals: the launch log keeps the pointer.
inline const char* sd_conv_label(int kernel, bool lockstep) {
  switch (kernel) {
    case SD_K_F32_S64_32: return "conv_gemm_f32_s64_kernel<32>";
    case SD_K_F32_S64_64: return "conv_gemm_f32_s64_kernel<64>";
    case SD_K_F32_SKINNY: return "skinny_gemm_f32_kernel";
    case SD_K_F32_T256: return "conv_gemm_f32_t256_kernel";
    case SD_K_F32_VH5: return "conv_gemm_f32_vh_kernel<5>";
    case SD_K_F32_VH6: return "conv_gemm_f32_vh_kernel<6>";
    case SD_K_F32_VH7: return "conv_gemm_f32_vh_kernel<7>";
    case SD_K_F32_N64: return "conv_gemm_f32_n64_kernel";
    case SD_K_F32_128: return "conv_gemm_f32_kernel<dma>";
    case SD_K_F32_128_SYMMETRIC: return "conv_gemm_f32_kernel<dma>/symmetric";
    case SD_K_F32_PACKED: return "conv_gemm_f32_packed_kernel";
    case SD_K_SEG_PARTIAL: return "seg_gemm_partial_f32_kernel";
    case SD_K_SEG_REDUCE: return "seg_gemm_reduce_f32_kernel";
    case SD_K_F16_128_HH: return "conv_gemm_f16_kernel<f16,f16>";
    case SD_K_F16_128_HF: return "conv_gemm_f16_kernel<f16,f32>";
    case SD_K_F16_128_FH: return "conv_gemm_f16_kernel<f32,f16>";
    case SD_K_F16_128_FF: return "conv_gemm_f16_kernel<f32,f32>";
    case SD_K_F16_T256_H_DIRECT: return lockstep ? "conv_gemm_f16_t256_kernel<f16,direct>/lockstep" : "conv_gemm_f16_t256_kernel<f16,direct>/grid";
    case SD_K_F16_T256_H_STAGED: return "conv_gemm_f16_t256_kernel<f16,staged>/grid";
    case SD_K_F16_T256_F_DIRECT: return lockstep ? "conv_gemm_f16_t256_kernel<f32,direct>/lockstep" : "conv_gemm_f16_t256_kernel<f32,direct>/grid";
    case SD_K_F16_T256_F_STAGED: return "conv_gemm_f16_t256_kernel<f32,staged>/grid";
    case SD_K_SPLIT_T256_DIRECT: return lockstep ? "conv_gemm_f16_t256_kernel<split,direct>/lockstep" : "conv_gemm_f16_t256_kernel<split,direct>/grid";
    case SD_K_SPLIT_T256_STAGED: return "conv_gemm_f16_t256_kernel<split,staged>/grid";
    default: return "conv_gemm_split16_n128_kernel";
  }
}

// One launch.  refuse != nullptr: the operator refuses the arguments (SD_ERR_ARG) with that text, and nothing else of the choice counts.
struct SdConvChoice {
  int kernel;            // SdConvKernel
  const char* label;
  long grid;
  int block;
  size_t lds;            // dynamic LDS bytes (0: none to allow)
  int prof;              // SD_PROF_* kind of the per-kernel timing, -1: outside it
  int stat_rows;         // the row unit of the column statistics the launch writes: 128, or 80 / 96 / 112 on a vh kernel
  int order, ntiles;     // the 128x128 f32 kernel: its walk (1; 2: the symmetric band list) and the length of its tile list
  int super_walk;        // the 256x256 f16 kernel: 1 = 256 persistent workgroups in lockstep
  int nsplit, groups;    // the seg_gemm pair: K splits over the grid, k-groups of 8 per wave
  const char* refuse;
};

// ---------------------------------------------------------------- geometry (each .hip file static_asserts these against its kernels)
constexpr int SD_T128 = 128;                       // the 128x128 kernels of both files
constexpr int SD_T256 = 256;                       // the 256x256 ring kernels of both files
constexpr int SD_F32_BK = 32;                      // floats per K step and staged row of the f32 kernels
constexpr int SD_S64 = 64, SD_S64_STAGES = 4;      // the 64x64 ring kernel
constexpr int SD_SKINNY = 32;                      // the 32x32 split-K kernel and the seg_gemm pair
constexpr size_t SD_LDS_F32_128 = (size_t)2 * (SD_T128 + SD_T128) * (SD_F32_BK + 4) * sizeof(float);   // the epilogue's C tile needs BM * LDC <= this
constexpr size_t SD_LDS_F32_N64 = (size_t)2 * (SD_T128 + 64) * SD_F32_BK * sizeof(float);
constexpr size_t SD_LDS_F32_S64 = (size_t)SD_S64_STAGES * 2 * SD_S64 * SD_F32_BK * sizeof(float);
constexpr size_t SD_LDS_T256 = 5 * SD_T256 * 128;                                 // three A stages + two B stages of 256 rows x 128 bytes
constexpr size_t SD_LDS_F16_128 = (size_t)2 * (SD_T128 + SD_T128) * (64 + 8) * 2;     // two stages of padded rows of 64 halfs
constexpr size_t sd_lds_f32_vh(int j) { return (size_t)2 * (16 * j + SD_T128) * SD_F32_BK * sizeof(float); }   // two stages of (16 J + BN) rows

// The floors of the column statistics (SdConvRule::colstat_T): a tile of 128 rows spans at most three segments from T = 64 on, a tile
// of 256 rows at most two from T = 128 on.  SD_STAT_UNIT_MIN: the smallest row unit a launch can write them in (the 80-row vh kernel).
constexpr int SD_COLSTAT_T_128 = 64, SD_COLSTAT_T_256 = 128, SD_STAT_UNIT_MIN = 80;

inline long sd_cdiv(long a, long b) { return (a + b - 1) / b; }
inline long sd_tiles(const sd_conv_args& a, int rows, int cols) { return sd_cdiv(a.M, rows) * sd_cdiv(a.cout, cols); }
inline bool sd_has_tee_add(const sd_conv_args& a) { return a.tee && a.tee_add; }

inline bool sd_refuse(SdConvChoice* c, const char* why) { c->refuse = why; return false; }
inline bool sd_fill(SdConvChoice* c, int kernel, long grid, int block, size_t lds, int prof, bool lockstep = false) {
  c->kernel = kernel; c->label = sd_conv_label(kernel, lockstep); c->grid = grid; c->block = block; c->lds = lds; c->prof = prof;
  return true;
}
inline SdConvChoice sd_no_choice() { SdConvChoice c = {}; c.stat_rows = 128; c.order = 1; return c; }

// ---------------------------------------------------------------- sd_conv1d_cl_f32 (and _symmetric, _rows)
// time-axis convs of small launches: 64x64 tiles through a 4-stage LDS-DMA ring (SD_TUNE_S64_TILES); 32-row tiles below 128 tiles
inline bool sd_f32_takes_ring(const sd_conv_args& a, bool symmetric, long t128, const SdConvTuning& t) {
  return !a.colstat && !symmetric && a.T > 1 && a.M >= SD_S64 && t128 < t.tune[SD_TUNE_S64_TILES];
}
inline bool sd_f32_ring_halves(long tiles64) { return tiles64 < 128; }
// fewer 128x128 tiles than half the CUs: 32x32 tiles with in-workgroup split-K (SD_TUNE_SKINNY_TILES)
inline bool sd_f32_takes_skinny(const sd_conv_args& a, long t128, const SdConvTuning& t) { return !a.colstat && t128 < t.tune[SD_TUNE_SKINNY_TILES]; }
// wide outputs of large launches: the 256x256 ring kernel (no tee_add epilogue, column statistics only for tiles that span <= 2
// segments, at least SD_TUNE_WIDE_TILES tiles: four rounds over the CUs)
inline bool sd_f32_takes_wide(const sd_conv_args& a, bool symmetric, long t256, const SdConvTuning& t) {
  return !symmetric && a.cout >= 1024 && t256 >= t.tune[SD_TUNE_WIDE_TILES] && t256 > 0 && !sd_has_tee_add(a) && !(a.colstat && a.T < SD_COLSTAT_T_256);
}
// 128x64 tiles are possible: not on the symmetric list; with column statistics only for T >= 128 and whole column tiles
inline bool sd_f32_can_halve(const sd_conv_args& a, bool symmetric, long t64) {
  return !symmetric && (!a.colstat || (a.T >= 128 && a.cout % 64 == 0)) && t64 < (1L << 31);
}
// Tiles of 16 J rows are possible.  T > 1: the time-axis convs.  The 16x16x4 MFMA sums four products per step where the 32x32x2 one sums
// two, so its results differ from the other kernels' in the last bit; plain products such as the affinity's row blocks (T = 1) keep the
// bits of the 128x128 kernel.  Column statistics in units of 16 J rows: only for a caller that asked for the unit.
inline bool sd_f32_can_vary_rows(const sd_conv_args& a, bool symmetric, bool takes_stat_rows) {
  return !symmetric && a.T > 1 && (!a.colstat || takes_stat_rows);
}
// ... and with column statistics a tile may span two (J = 5) / three segments
inline bool sd_f32_vh_stat_ok(const sd_conv_args& a, int j) { return !(a.colstat && a.T < (j == 5 ? SD_STAT_UNIT_MIN : 8 * j)); }

inline bool sd_choose_conv_f32(const sd_conv_args& a, int vec, bool symmetric, bool takes_stat_rows, const SdConvTuning& t, SdConvChoice* c) {
  (void)vec;
  *c = sd_no_choice();
  const long tiles_m = sd_cdiv(a.M, SD_T128), tiles_n = sd_cdiv(a.cout, SD_T128), t128 = tiles_m * tiles_n;
  if (!(t128 < (1L << 31))) return sd_refuse(c, "sd_conv1d_cl_f32: grid too large");
  if (sd_f32_takes_ring(a, symmetric, t128, t)) {
    const long nt64 = sd_cdiv(a.cout, SD_S64), g = sd_cdiv(a.M, SD_S64) * nt64;
    if (sd_f32_ring_halves(g)) return sd_fill(c, SD_K_F32_S64_32, sd_cdiv(a.M, 32) * nt64, 256, SD_LDS_F32_S64, -1);
    return sd_fill(c, SD_K_F32_S64_64, g, 256, SD_LDS_F32_S64, -1);
  }
  // (not counted in the SD_PROF_CONV_GEMM roofline figures: a different kernel, 0.2 % of the flops)
  if (sd_f32_takes_skinny(a, t128, t)) return sd_fill(c, SD_K_F32_SKINNY, sd_tiles(a, SD_SKINNY, SD_SKINNY), 256, 0, -1);
  const long t256 = sd_tiles(a, SD_T256, SD_T256);
  if (sd_f32_takes_wide(a, symmetric, t256, t)) return sd_fill(c, SD_K_F32_T256, t256, 512, SD_LDS_T256, SD_PROF_CONV_WIDE);
  // Half-width tiles when they shorten the busiest CU's share (SD_TUNE_HALF_TILES).  Measured (tools/probe_tile_alone.py): a launch takes
  // ~15 us + (tiles on the busiest CU) x 62 us per unit of K = 1024, whether the CU's tiles run side by side or one after the other; a
  // half tile costs 0.52 of a tile.  The rounds are those of the MI355X's 256 CUs whatever the device.
  const long half = t.tune[SD_TUNE_HALF_TILES], rows = t.tune[SD_TUNE_TILE_ROWS];
  const long t64 = tiles_m * sd_cdiv(a.cout, 64);
  const double cost128 = (double)sd_cdiv(t128, 256), cost64 = 0.52 * (double)sd_cdiv(t64, 256);
  const bool can = sd_f32_can_halve(a, symmetric, t64);
  // tiles of 80 / 96 / 112 rows (SD_TUNE_TILE_ROWS): a tile of 16 J rows costs J / 8 of a 128-row tile
  int best = 0;
  double best_cost = 0.97 * (half != 0 && can && cost64 < cost128 ? cost64 : cost128);
  if (sd_f32_can_vary_rows(a, symmetric, takes_stat_rows) && rows != 0)
    for (int j = 5; j <= 7; ++j) {
      if (!sd_f32_vh_stat_ok(a, j)) continue;
      const double cj = (double)sd_cdiv(sd_cdiv(a.M, 16 * j) * tiles_n, 256) * (double)j / 8.0 * 1.02;
      if (rows == 16 * j || (rows < 0 && cj < best_cost)) { best = j; best_cost = cj; }
    }
  if (best) {
    c->stat_rows = 16 * best;
    return sd_fill(c, SD_K_F32_VH5 + (best - 5), sd_cdiv(a.M, 16 * best) * tiles_n, 256, sd_lds_f32_vh(best), SD_PROF_CONV_GEMM);
  }
  if (can && half != 0 && (half == 1 || cost64 < 0.97 * cost128)) return sd_fill(c, SD_K_F32_N64, t64, 256, SD_LDS_F32_N64, SD_PROF_CONV_GEMM);
  // the 128x128 kernel, one workgroup per entry of its tile list: every tile, or the band entries on and above the diagonal
  c->ntiles = (int)t128;
  if (symmetric && tiles_n >= 2) {
    long n = 0;
    for (long b = 0; 8 * b < tiles_n; ++b) n += (tiles_n - 8 * b < 8 ? tiles_n - 8 * b : 8) * (tiles_n - 8 * b);
    c->ntiles = (int)n;
    c->order = 2;
  }
  return sd_fill(c, symmetric ? SD_K_F32_128_SYMMETRIC : SD_K_F32_128, c->ntiles, 256, SD_LDS_F32_128, SD_PROF_CONV_GEMM);
}

// Packed spans: the 128x128 kernel's packed form, whatever the tuning selects for uniform launches (no other kernel has the span map)
inline bool sd_choose_conv_packed(const sd_conv_args& a, int vec, const SdConvTuning& t, SdConvChoice* c) {
  (void)vec; (void)t;
  *c = sd_no_choice();
  const long tiles = sd_tiles(a, SD_T128, SD_T128);
  if (!(tiles < (1L << 31))) return sd_refuse(c, "sd_conv1d_cl_packed_f32: grid too large");
  return sd_fill(c, SD_K_F32_PACKED, tiles, 256, SD_LDS_F32_128, SD_PROF_CONV_GEMM);
}

// ---------------------------------------------------------------- sd_seg_gemm_f32
// The grid split-K of a per-segment layer: a split = 4 waves x `groups` k-groups of 8, i.e. 256 values of K for the long layers, 128
// below 2048.  0: the shape does not split (too many rows, K short or ragged, fewer than two splits).
inline int sd_seg_gemm_shape(int M, int cin_pad, int cout, int* groups, int* nsplit, long* tiles) {
  if (M <= 0 || M > 256 || cin_pad < 512 || cin_pad % 32 != 0 || cout <= 0) return 0;
  *groups = cin_pad >= 2048 ? 8 : 4;
  *nsplit = (int)(((long)cin_pad + 32 * *groups - 1) / (32 * *groups));
  *tiles = sd_cdiv(M, SD_SKINNY) * sd_cdiv(cout, SD_SKINNY);
  return *nsplit >= 2;
}
inline size_t sd_seg_gemm_scratch(long tiles, int nsplit) { return (size_t)tiles * nsplit * SD_SKINNY * SD_SKINNY * sizeof(float); }

// K split over the grid when the launch is small and K long (two launches: partial sums into the caller's scratch, then the reduction
// with the epilogue), otherwise what sd_conv1d_cl_f32 chooses.  scratch_ok: the caller's scratch is non-null and 16-byte aligned.
// Returns the number of launches in c[] (0: refused, c[0].refuse says why).
inline int sd_choose_seg_gemm(const sd_conv_args& a, int vec, bool scratch_ok, size_t scratch_bytes, const SdConvTuning& t, SdConvChoice c[2]) {
  int groups = 0, nsplit = 0;
  long tiles = 0;
  const bool per_segment = a.T == 1 && a.taps == 1 && !a.tee && !a.colstat;
  if (!(per_segment && scratch_ok && sd_seg_gemm_shape(a.M, a.cin_pad, a.cout, &groups, &nsplit, &tiles) && sd_seg_gemm_scratch(tiles, nsplit) <= scratch_bytes))
    return sd_choose_conv_f32(a, vec, false, false, t, &c[0]) ? 1 : 0;
  c[0] = c[1] = sd_no_choice();
  c[0].nsplit = c[1].nsplit = nsplit;
  c[0].groups = c[1].groups = groups;
  sd_fill(&c[0], SD_K_SEG_PARTIAL, tiles * nsplit, 256, 0, SD_PROF_SEG_SPLITK);
  sd_fill(&c[1], SD_K_SEG_REDUCE, tiles * 4, 256, 0, -1);
  return 2;
}

// ---------------------------------------------------------------- sd_conv1d_cl_f16, sd_conv1d_cl_split16
// Small launches of the C-wide layers.  f16 (round 3, tools/sweep_f16.py): 1024 -> 1024 at 16 / 32 segments 0.024 / 0.030 ms on the
// 128x128 kernel against 0.035 / 0.038 on the 256x256 one.  split16 (tools/probe_split16.py): at 32 segments 0.063 ms on the 128x128
// split kernel against 0.085 ms for pack + 256x256 kernel, 0.041 against 0.079 at 16.  From 64 segments up, and for 3C -> 3C always, the
// 256x256 kernel wins: at most SD_TUNE_F16_NARROW_TILES (128) tiles of 256x256 and cout <= 1024 -> two workgroups of 128x128 per CU
// fill the chip better than a fraction of one round of big tiles.  (The narrow split kernel has no column statistics.)
inline bool sd_wide_goes_narrow(int cout, int M, long narrow_tiles) {
  return cout <= 1024 && sd_cdiv(M, SD_T256) * sd_cdiv(cout, SD_T256) <= narrow_tiles;
}
// the register ("direct") epilogue of the 256x256 kernel: relu / identity with a per-channel bias, no tee, aligned slices
inline bool sd_t256_plain(const sd_conv_args& a, int vec) {
  return vec && (a.act == SD_ACT_RELU || a.act == SD_ACT_NONE) && a.act2 == SD_ACT_NONE && !a.bias_per_seg && !a.tee;
}
// The 256x256 kernel's walk.  Lockstep (256 persistent workgroups, 8 x 4 tiles per XCD and pass) when the tile list is several rounds
// long, the chip has 8 x 32 CUs and the column tiles come in fours (SD_TUNE_T256_LOCKSTEP_TILES: from how many tiles; default 4 x 256);
// else one workgroup per tile.
inline bool sd_fill_t256(const sd_conv_args& a, int kernel, bool direct, const SdConvTuning& t, SdConvChoice* c) {
  const long tiles_n = sd_cdiv(a.cout, SD_T256), total = sd_cdiv(a.M, SD_T256) * tiles_n;
  const long from = t.tune[SD_TUNE_T256_LOCKSTEP_TILES] < 0 ? 4L * 256 : t.tune[SD_TUNE_T256_LOCKSTEP_TILES];
  const bool lockstep = direct && t.n_cu == 256 && tiles_n % 4 == 0 && total < (1L << 30) && total >= from;
  c->super_walk = lockstep ? 1 : 0;
  return sd_fill(c, kernel, lockstep ? 256L : total, 512, SD_LDS_T256, SD_PROF_CONV_WIDE, lockstep);
}

// Measured per shape on MI355X (tools/probe_conv.py, B*T = 1 005 000 rows): the 256x256 LDS-DMA kernel wins wherever the output is
// wide (3072x3072: 987 vs ~800 TFLOP/s, 1024x1024: 789 vs 726, 128->3072: 342 vs 315); the register-staged 128x128 kernel with two
// workgroups per CU is faster on the narrow outputs (Res2Net 128x384: 555, 3072->128: 530 vs 408) and is the only one with the tee_add
// epilogue.  The 256x256 kernel reads f16 x only, and writes column statistics only for tiles that span <= 2 segments.
inline bool sd_f16_takes_wide(const sd_conv_args& a, const SdConvTuning& t) {
  const bool wide = a.cout >= 1024 && !sd_wide_goes_narrow(a.cout, a.M, t.tune[SD_TUNE_F16_NARROW_TILES]);
  return a.x_dtype == SD_DT_F16 && (t.f16_kernel >= 0 ? t.f16_kernel == 2 : wide) && !sd_has_tee_add(a) && !(a.colstat && a.T < SD_COLSTAT_T_256);
}
inline bool sd_choose_conv_f16(const sd_conv_args& a, int vec, const SdConvTuning& t, SdConvChoice* c) {
  *c = sd_no_choice();
  if (!(sd_tiles(a, SD_T128, SD_T128) < (1L << 31))) return sd_refuse(c, "sd_conv1d_cl_f16: grid too large");
  const bool xa = a.x_dtype == SD_DT_F16, ya = a.y_dtype == SD_DT_F16;
  if (sd_f16_takes_wide(a, t)) {
    const bool direct = sd_t256_plain(a, vec) && t.t256_direct;
    return sd_fill_t256(a, ya ? (direct ? SD_K_F16_T256_H_DIRECT : SD_K_F16_T256_H_STAGED) : (direct ? SD_K_F16_T256_F_DIRECT : SD_K_F16_T256_F_STAGED), direct, t, c);
  }
  return sd_fill(c, xa ? (ya ? SD_K_F16_128_HH : SD_K_F16_128_HF) : (ya ? SD_K_F16_128_FH : SD_K_F16_128_FF), sd_tiles(a, SD_T128, SD_T128), 256,
                 SD_LDS_F16_128, SD_PROF_CONV_GEMM);
}

// x plain f32 (split while staged): the 128x128 kernel.  x SD_DT_SPLIT16: the 256x256 kernel; y as split halves comes from the LDS-staged
// epilogue's store phase (the register epilogue writes f32 only).
inline bool sd_choose_conv_split16(const sd_conv_args& a, int vec, const SdConvTuning& t, SdConvChoice* c) {
  *c = sd_no_choice();
  if (a.x_dtype == SD_DT_F32) {
    const long tiles = sd_tiles(a, SD_T128, SD_T128);
    if (!(tiles < (1L << 31))) return sd_refuse(c, "sd_conv1d_cl_split16: grid too large");
    return sd_fill(c, SD_K_SPLIT_N128, tiles, 256, SD_LDS_F16_128, SD_PROF_CONV_GEMM);
  }
  if (!(sd_tiles(a, SD_T256, SD_T256) < (1L << 31))) return sd_refuse(c, "sd_conv1d_cl_split16: grid too large");
  const bool direct = a.y_dtype != SD_DT_SPLIT16 && sd_t256_plain(a, vec);
  return sd_fill_t256(a, direct ? SD_K_SPLIT_T256_DIRECT : SD_K_SPLIT_T256_STAGED, direct, t, c);
}
