// The choice layer alone: csrc/sd_conv_choice.h in a plain C++ program (no HIP header, no library), built with the address and
// undefined-behaviour sanitizers by tests/test_conv_choice_rules.py.  It calls every sd_choose_* over the corners of the sweep -- M from
// 1 to 2^31 - 1, cout from 1 -- under the default tuning and under every pin, and checks what any caller relies on: a label, a grid of
// at least one workgroup, or a refusal with its text.  Prints the number of choices made.
#ifdef __HIP__
#error "the choice must compile without HIP"
#endif
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "sd_conv_choice.h"

static long g_choices = 0;

static void expect(const SdConvChoice& c, bool ok, const char* what) {
  ++g_choices;
  const bool fine = ok ? (c.label && c.grid >= 1 && c.block > 0 && !c.refuse && c.stat_rows >= 80 && c.stat_rows <= 128) : c.refuse != nullptr;
  if (!fine) {
    fprintf(stderr, "%s: ok=%d label=%s grid=%ld refuse=%s\n", what, (int)ok, c.label ? c.label : "(null)", c.grid, c.refuse ? c.refuse : "(null)");
    exit(1);
  }
}

int main() {
  static float mem[64];
  void* const some = mem;                 // never dereferenced: a choice reads null / not null only
  const int Ms[] = {1, 31, 32, 33, 64, 127, 128, 129, 255, 256, 257, 70000, 1 << 20, 2147483647};
  const int couts[] = {1, 8, 40, 64, 128, 1016, 1024, 1536, 3072};
  const int Ts[] = {1, 5, 64, 79, 80, 127, 128, 201};
  const long pins[][2] = {{0, 0}, {SD_TUNE_S64_TILES, 0}, {SD_TUNE_SKINNY_TILES, 0}, {SD_TUNE_WIDE_TILES, 0}, {SD_TUNE_HALF_TILES, 1}, {SD_TUNE_HALF_TILES, 0},
                          {SD_TUNE_TILE_ROWS, 80}, {SD_TUNE_TILE_ROWS, 112}, {SD_TUNE_TILE_ROWS, 0}, {SD_TUNE_F16_NARROW_TILES, 0}, {SD_TUNE_T256_LOCKSTEP_TILES, 0},
                          {SD_TUNE_SKINNY_TILES, 1L << 40}, {SD_TUNE_S64_TILES, 1L << 40}};
  for (const auto& pin : pins)
    for (int n_cu : {0, 256}) {
      SdConvTuning t = sd_conv_tuning_default(n_cu);
      if (pin[0]) t.tune[pin[0]] = sd_tune_stored((int)pin[0], pin[1]);
      for (int M : Ms)
        for (int cout : couts)
          for (int T : Ts)
            for (int flags = 0; flags < 8; ++flags) {
              sd_conv_args a = {};
              a.x = a.w = some; a.y = some;
              a.M = M; a.T = T; a.cin = 64; a.cin_pad = flags & 4 ? 2048 : 64; a.cout = cout; a.taps = 1; a.dil = 1;
              a.lda = a.cin; a.ldo = cout;
              if (flags & 1) a.colstat = mem;
              if (flags & 2) { a.tee = some; a.tee_add = some; a.tee_hi = 1; a.ldt = 1; a.ld_ta = 1; }
              SdConvChoice c[2];
              for (int vec = 0; vec < 2; ++vec) {
                for (int sym = 0; sym < 2; ++sym)
                  for (int rows = 0; rows < 2; ++rows) expect(c[0], sd_choose_conv_f32(a, vec, sym != 0, rows != 0, t, &c[0]), "f32");
                expect(c[0], sd_choose_conv_packed(a, vec, t, &c[0]), "packed");
                const int n = sd_choose_seg_gemm(a, vec, (flags & 4) != 0, flags & 4 ? (size_t)1 << 40 : 0, t, c);
                expect(c[0], n > 0, "seg_gemm");
                if (n == 2) expect(c[1], true, "seg_gemm reduce");
                for (int xd : {SD_DT_F32, SD_DT_F16})
                  for (int yd : {SD_DT_F32, SD_DT_F16}) {
                    a.x_dtype = xd; a.y_dtype = yd; a.w_dtype = SD_DT_F16;
                    expect(c[0], sd_choose_conv_f16(a, vec, t, &c[0]), "f16");
                  }
                for (int xd : {SD_DT_F32, SD_DT_SPLIT16})
                  for (int yd : {SD_DT_F32, SD_DT_SPLIT16}) {
                    a.x_dtype = xd; a.y_dtype = yd; a.w_dtype = SD_DT_SPLIT16;
                    expect(c[0], sd_choose_conv_split16(a, vec, t, &c[0]), "split16");
                  }
                a.x_dtype = a.y_dtype = a.w_dtype = SD_DT_F32;
              }
            }
    }
  // the one refusal a choice makes: more 128x128 tiles than a grid holds
  sd_conv_args big = {};
  big.M = 2147483647; big.T = 1; big.cout = 1 << 20; big.cin = big.cin_pad = 64; big.taps = big.dil = 1;
  SdConvChoice c[2];
  const SdConvTuning t = sd_conv_tuning_default(256);
  expect(c[0], sd_choose_conv_f32(big, 1, false, false, t, &c[0]), "f32 too large");
  expect(c[0], sd_choose_conv_packed(big, 1, t, &c[0]), "packed too large");
  expect(c[0], sd_choose_conv_f16(big, 1, t, &c[0]), "f16 too large");
  expect(c[0], sd_choose_conv_split16(big, 1, t, &c[0]), "split16 too large");
  expect(c[0], sd_choose_seg_gemm(big, 1, true, 0, t, c) > 0, "seg_gemm too large");
  printf("%ld choices\n", g_choices);
  return 0;
}
