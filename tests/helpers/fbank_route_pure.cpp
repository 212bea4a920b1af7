// The fbank check and route alone: csrc/sd_fbank_route.h in a plain C++ program (no HIP header, no library), built with the address
// and undefined-behaviour sanitizers by tests/test_fbank_route_rules.py.  Every argument is one call,
//     form:plan:n_mels:switch:B:n:n_total:M:ld_out:ws_bytes:nulls
// (form u / l / w / p; plan sb = 400 / 160 zero-padded dB, ta = 400 / 160 reflect ln, g8 = 200 / 80; n_total -1: B n; ws_bytes -1: what
// the call needs; nulls: letters of p w o s l f k (plan, wav, out, starts, lens, frame_start, workspace) and m for a misaligned
// workspace), answered by one line: the status, and the refusal or the route.  "sweep:B": (B, n) for n = 1 .. 40 000 on the sb plan,
// one short line each.
#ifdef __HIP__
#error "the route must compile without HIP"
#endif
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "sd_fbank_route.h"

static SdFbankFacts plan_facts(const char* plan, int n_mels, bool on) {
  const bool generic = !strcmp(plan, "g8"), speechbrain = !strcmp(plan, "sb");
  SdFbankFacts f = {};
  f.n_fft = generic ? 200 : 400;
  f.hop = generic ? 80 : 160;
  f.n_mels = n_mels;
  f.pad_mode = speechbrain ? SD_PAD_ZERO : SD_PAD_REFLECT;
  f.log_mode = speechbrain ? SD_LOG_DB_TOPDB : SD_LOG_LN_EPS;
  f.log_eps = speechbrain ? 1e-10f : 1e-6f;
  f.top_db = speechbrain ? 80.f : -1.f;
  f.generic = generic;
  f.utt_tables = !generic;
  f.utt_switch = on;
  f.fold_threads = 512;        // the shipped build: SD_FB_GROUPS = 2
  f.fold_lds = 152576;
  return f;
}

static void print_launch(const char* name, const SdFbankLaunch& l) { printf(" %s=%ld/%d/%zu", name, l.grid, l.block, l.lds); }

static void answer(const SdFbankFacts& f, const SdFbankCall& c) {
  SdFbankRoute r;
  char why[SD_FB_WHY] = "";
  const int status = sd_fbank_check(f, c, &r, why);
  if (status != SD_OK) {
    printf("status=%d why=%s\n", status, why);
    return;
  }
  printf("status=0 kinds=%d T=%d flat=%d tiles=%ld n_cap=%d n_lo=%d use_floor=%d inv_mels=%u inv_row=%u R=%d maxkey=%zu tile_off=%zu ws_need=%zu", r.kinds, r.T,
         r.flat, r.tiles, r.n_cap, r.n_lo, r.use_floor, r.inv_mels, r.inv_row, r.R, r.maxkey_bytes, r.tile_table_off, r.ws_need);
  print_launch("utt16", r.utt16);
  print_launch("fill", r.fill);
  print_launch("tile_table", r.tile_table);
  print_launch("logmel", r.logmel);
  print_launch("finalize", r.finalize);
  printf(" uniform_ws=%zu packed_ws=%zu\n", sd_fbank_uniform_ws_bytes(f, c.B, c.n), sd_fbank_packed_ws_bytes(c.B));
}

int main(int argc, char** argv) {
  static const char* const entries[] = {"sd_fbank_f32", "sd_fbank_lens_f32", "sd_fbank_windows_f32", "sd_fbank_packed_f32"};
  for (int i = 1; i < argc; ++i) {
    int B = 0;
    if (sscanf(argv[i], "sweep:%d", &B) == 1) {
      const SdFbankFacts f = plan_facts("sb", 80, true);
      for (int n = 1; n <= 40000; ++n) {
        SdFbankCall c = {};
        c.entry = entries[0]; c.form = SD_FB_UNIFORM; c.B = B; c.n = n; c.n_total = (long long)B * n; c.mean_norm = 1; c.ld_out = 80; c.ws_bytes = (size_t)1 << 30;
        c.no_starts = c.no_lens = c.no_frame_start = true;
        const SdFbankRoute r = sd_fbank_route(f, c);
        printf("%d %d %d %d %d %ld %ld %ld %d %d %zu\n", B, n, r.kinds, r.T, r.flat, r.tiles, r.utt16.grid, r.logmel.grid, r.R, r.finalize.block, r.utt16.lds);
      }
      continue;
    }
    char form = 0, plan[8] = "", nulls[16] = "";
    int n_mels = 0, on = 0, n = 0, M = 0, ld_out = 0;
    long long n_total = 0, ws = 0;
    if (sscanf(argv[i], "%c:%7[^:]:%d:%d:%d:%d:%lld:%d:%d:%lld:%15s", &form, plan, &n_mels, &on, &B, &n, &n_total, &M, &ld_out, &ws, nulls) < 10) {
      fprintf(stderr, "bad call: %s\n", argv[i]);
      return 2;
    }
    const int f_id = form == 'u' ? SD_FB_UNIFORM : form == 'l' ? SD_FB_LENS : form == 'w' ? SD_FB_WINDOWS : SD_FB_PACKED;
    const SdFbankFacts f = strchr(nulls, 'p') ? SdFbankFacts{} : plan_facts(plan, n_mels, on != 0);
    const bool packed = f_id == SD_FB_PACKED;
    if (n_total < 0) n_total = (long long)B * n;
    const size_t need = packed ? sd_fbank_packed_ws_bytes(B) : sd_fbank_uniform_ws_bytes(f, B, n);
    const auto no = [&](char k) { return strchr(nulls, k) != nullptr; };
    SdFbankCall c = {};
    c.entry = entries[f_id]; c.form = f_id; c.B = B; c.n = n; c.n_total = n_total; c.M = M;
    c.mean_norm = form == 'l' || packed ? 1 : 0; c.ld_out = ld_out; c.ws_bytes = ws < 0 ? need : (size_t)ws;
    c.no_plan = no('p'); c.no_wav = no('w'); c.no_out = no('o'); c.no_ws = no('k'); c.ws_misaligned = no('m');
    c.no_starts = f_id == SD_FB_WINDOWS || packed ? no('s') : true;       // (an entry without the pointer passes none)
    c.no_lens = packed ? no('l') : true;
    c.no_frame_start = packed ? no('f') : true;
    answer(f, c);
  }
  return 0;
}
