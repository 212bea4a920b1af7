// The checks of sd_vad_energy_grouped_f32 and sd_vad_segments_grouped, alone: csrc/vad/sd_vad_check.h in a plain C++ program (no HIP
// header, no library), built with the address and undefined-behaviour sanitizers by tests/test_vad_rules.py.  Every argument is one call:
//     energy:n_groups:n_frames:n_signal:win:hop:threshold_db:slope:flags          flags: letters of t = a null table pointer,
//                                                                                  f = null signal or probs, or -
//     segments:n_groups:n_frames:seg_cap:on:off:open_len:close_len:min_run:max_gap:ws_bytes:flags
//                                                                                  ws_bytes -1: what the call needs; flags: t = a null table
//                                                                                  pointer, p = null probs, s = null seg_start, seg_end or
//                                                                                  ws, m = a misaligned workspace, or -
// (floats as strtod reads them, "nan" and "inf" included), answered by one line: "status=0 need=BYTES" or "status=CODE why=TEXT".
// "size:seg_cap:n_groups" prints what sd_vad_segments_workspace_bytes returns, "stage:count:win:hop" the floats a tile stages,
// "layout" the constants of the two kernels, "cap:n" the run capacity of n frames.
#ifdef __HIP__
#error "the check must compile without HIP"
#endif
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "vad/sd_vad_check.h"

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    int g = 0, nf = 0, cap = 0, win = 0, hop = 0, ol = 0, cl = 0, mr = 0, mg = 0, count = 0;
    long long ns = 0, ws = 0;
    char a[32] = "", b[32] = "", flags[8] = "";
    if (sscanf(argv[i], "size:%d:%d", &cap, &g) == 2) {
      printf("%zu\n", sd_vad_workspace_bytes(cap, g));
      continue;
    }
    if (sscanf(argv[i], "stage:%d:%d:%d", &count, &win, &hop) == 3) {
      printf("%ld\n", sd_vad_stage_floats(count, win, hop));
      continue;
    }
    if (sscanf(argv[i], "cap:%d", &nf) == 1) {
      printf("%d\n", sd_vad_run_capacity(nf));
      continue;
    }
    if (strcmp(argv[i], "layout") == 0) {
      printf("%d %d %d %d %d %d\n", SD_VAD_E_THREADS, SD_VAD_E_TILE, SD_VAD_E_STAGE, SD_VAD_S_THREADS, SD_VAD_S_LDS_RUNS, SD_VAD_S_LDS_FRAMES);
      continue;
    }
    char why[SD_VAD_WHY] = "";
    if (sscanf(argv[i], "energy:%d:%d:%lld:%d:%d:%31[^:]:%31[^:]:%7s", &g, &nf, &ns, &win, &hop, a, b, flags) == 8) {
      SdVadEnergyCall c = {};
      c.n_groups = g, c.n_frames = nf, c.n_signal = ns, c.win = win, c.hop = hop;
      c.threshold_db = strtof(a, nullptr), c.slope = strtof(b, nullptr);
      c.table_null = strchr(flags, 't') != nullptr;
      c.frames_null = strchr(flags, 'f') != nullptr;
      const int status = sd_vad_energy_check(c, why);
      if (status != SD_OK) printf("status=%d why=%s\n", status, why);
      else printf("status=0 need=0\n");
      continue;
    }
    if (sscanf(argv[i], "segments:%d:%d:%d:%31[^:]:%31[^:]:%d:%d:%d:%d:%lld:%7s", &g, &nf, &cap, a, b, &ol, &cl, &mr, &mg, &ws, flags) == 11) {
      SdVadSegmentsCall c = {};
      c.n_groups = g, c.n_frames = nf, c.seg_cap = cap, c.open_len = ol, c.close_len = cl, c.min_run = mr, c.max_gap = mg;
      c.on = strtof(a, nullptr), c.off = strtof(b, nullptr);
      c.table_null = strchr(flags, 't') != nullptr;
      c.probs_null = strchr(flags, 'p') != nullptr;
      c.segs_null = strchr(flags, 's') != nullptr;
      c.ws_misaligned = strchr(flags, 'm') != nullptr;
      c.ws_bytes = ws >= 0 ? (size_t)ws : (sd_vad_segments_check(c, why, true) == SD_OK ? sd_vad_segments_need(c) : 0);
      const int status = sd_vad_segments_check(c, why);
      if (status != SD_OK) printf("status=%d why=%s\n", status, why);
      else printf("status=0 need=%zu\n", sd_vad_segments_need(c));
      continue;
    }
    fprintf(stderr, "bad call: %s\n", argv[i]);
    return 2;
  }
  return 0;
}
