// What a fbank entry refuses and what it launches: CHECK and ROUTE, pure and host-only.  The four entries of
// sd_fbank.hip describe their call (SdFbankCall), hand it with the plan's facts (SdFbankFacts) to sd_fbank_check and launch what the
// SdFbankRoute says.  Nothing else is read: no device pointer, no environment (SD_FBANK_UTT comes in as a fact), no device query.
// No HIP header, so the same functions compile into a plain C++ program (tests/test_fbank_route_rules.py).  Labels stay at the launch sites.
#pragma once
#include <stddef.h>
#include <stdio.h>

#include "sd_hip.h"

namespace sd_fb {
// ---------------------------------------------------------------- the kernels' constants (the 16 kHz framing; each file's own geometry)
constexpr int NFFT = 400, HOP = 160, NFREQ = 201;
constexpr int MELP = 81;                // row stride of the log-mel rows both kernels stage in LDS
// the one-launch kernel (sd_fbank_utt16.hip): LDS = resident matrix + table ring + scratch + the padded, skewed signal (word i + i / 160
// of n + 400 samples), which the utterance's log-mel rows later overwrite
constexpr int U16_MAX_T = 208;          // 13 tiles: two rounds of the 8 waves
constexpr int U16_THREADS = 512;
constexpr int A2_BYTES = 16 * 1024;
constexpr int RING_BYTES = 16 * 1024;   // two chunks of eight 1 KB fragments: the streamed tables, shared by the eight waves
constexpr int SCRATCH_FLOATS = 64;      // [0..15] wave maxima of the log-mel rows, [16..23] of |x|, [24..31] "this wave saw a NaN sample"
constexpr int LDS_LIMIT = 160 * 1024;
// the folded-DFT kernel (sd_fbank.hip static_asserts these against its own): a workgroup takes FOLD_WAVES tiles of FOLD_FT frames; its
// block and LDS size follow the build's SD_FB_GROUPS and come in as plan facts
constexpr int FOLD_FT = 32, FOLD_WAVES = 4;
constexpr size_t FBG_CHUNK_BYTES = (size_t)256 << 20;      // sd_fbank_generic.hip: the workspace of one chunk of utterances stays below
// ---------------------------------------------------------------- host arithmetic
constexpr int frames(int n) { return 1 + n / HOP; }
constexpr unsigned recip32(int x) { return (unsigned)((((unsigned long long)1 << 32) + x - 1) / x); }      // ceil(2^32 / x): e / x = umulhi(e, .) for e < 2^16
constexpr long cdiv(long a, long b) { return (a + b - 1) / b; }
constexpr int round_up(int v, int m) { return (v + m - 1) / m * m; }
constexpr size_t round256(size_t v) { return (v + 255) & ~(size_t)255; }
constexpr int fbg_nfp(int n_fft) { return round_up(n_fft / 2 + 1, 32); }      // 32 bins = one 64-column tile of the generic DFT kernel; the mel product's K step
constexpr int img_words(int n) { return (n + NFFT) + (n + NFFT) / HOP + 1; }
constexpr size_t u16_lds_bytes(int n) {
  const size_t img = (size_t)img_words(n), rows = (size_t)frames(n) * MELP;
  return (size_t)A2_BYTES + RING_BYTES + SCRATCH_FLOATS * 4 + (img > rows ? img : rows) * 4;
}
constexpr bool u16_fits(int n) { return frames(n) <= U16_MAX_T && u16_lds_bytes(n) <= (size_t)LDS_LIMIT; }
// the one-launch kernel's longest utterance (u16_lds_bytes is monotone): 16 384 + 16 384 + 256 + 4 * 32 704 = 163 840 there; 201 frames
constexpr int U16_MAX_N = 32100;
static_assert(u16_fits(U16_MAX_N) && !u16_fits(U16_MAX_N + 1) && u16_lds_bytes(U16_MAX_N) == (size_t)LDS_LIMIT && img_words(U16_MAX_N) == 32704, "");
}  // namespace sd_fb

// What a plan is, apart from its device tables: sd_fbank_plan_create sets these, once.
struct SdFbankFacts {
  int n_fft, hop, n_mels, pad_mode, log_mode;
  float log_eps, top_db;
  bool generic;          // any framing but 400 / 160 with at most 80 mels: sd_fbank_generic.hip
  bool utt_tables;       // the one-launch kernel's tables exist
  bool utt_switch;       // A/B: SD_FBANK_UTT=0 (behind SD_EXPERIMENT) sends every length to the folded kernel
  int fold_threads;      // the folded kernel's workgroup as built: 256 SD_FB_GROUPS threads (512 as shipped) ...
  size_t fold_lds;       // ... and its dynamic LDS bytes (152 576 as shipped)
};

enum SdFbankForm { SD_FB_UNIFORM, SD_FB_LENS, SD_FB_WINDOWS, SD_FB_PACKED };
// One call.  n: samples per row (packed: n_max).  n_total: samples behind `wav` (uniform and lens: B n).  entry: the name in front of a refusal.
struct SdFbankCall {
  const char* entry;
  int form, B, n;
  long long n_total;
  int M, mean_norm, ld_out;
  size_t ws_bytes;
  bool no_plan, no_wav, no_out, no_starts, no_lens, no_frame_start, no_ws, ws_misaligned;
};

struct SdFbankLaunch { long grid; int block; size_t lds; };     // grid 0: not launched
enum { SD_FB_GENERIC = 1, SD_FB_ONE_LAUNCH = 2, SD_FB_FOLDED = 4 };
struct SdFbankRoute {
  int kinds;             // 0: nothing to do (B = 0); a pack with spans on both sides of the boundary: SD_FB_ONE_LAUNCH | SD_FB_FOLDED
  int T, use_floor;      // T: frames of n (packed: of n_max)
  int n_cap;             // one-launch: spans of up to n_cap samples (uniform: n)
  unsigned inv_row;      // ... of the floats or float4s of an output row
  SdFbankLaunch utt16;
  int n_lo, flat;        // folded: spans of more than n_lo samples; tiles flat over (utterance, frame)
  long tiles;
  unsigned inv_mels;
  int R;                 // the finalize pass: thread (r, c) walks rows r, r + R, ... of mel c
  SdFbankLaunch fill, tile_table, logmel, finalize;
  size_t maxkey_bytes, tile_table_off, ws_need;      // the workspace: [max keys: B ints][packed: tile_start: B + 1 ints]
  int g_nfp, g_nmp, g_Lp, g_Bc;                      // generic: Bc utterances per chunk, each Lp padded samples + T (nfp + nmp) floats
};

inline size_t sd_fbank_maxkey_bytes(int B) { return sd_fb::round256((size_t)(B > 0 ? B : 0) * sizeof(int)); }
inline size_t sd_fbank_packed_ws_bytes(int B) { return B <= 0 ? 0 : sd_fbank_maxkey_bytes(B) + sd_fb::round256(((size_t)B + 1) * sizeof(int)); }

// frames of torch.stft(center = True): 1 + (n + 2 (n_fft / 2) - n_fft) / hop  (= 1 + n / hop for an even n_fft)
inline int sd_fbank_frames(const SdFbankFacts& f, int n) {
  const long long padded = (long long)n + 2 * (f.n_fft / 2);
  return padded < f.n_fft ? 0 : (int)(1 + (padded - f.n_fft) / f.hop);
}

// the generic route's numbers for (B, n)
inline void sd_fbank_generic_layout(const SdFbankFacts& f, int B, int n, SdFbankRoute* r) {
  r->T = sd_fbank_frames(f, n);
  r->g_nfp = sd_fb::fbg_nfp(f.n_fft);
  r->g_nmp = sd_fb::round_up(f.n_mels, 4);
  const size_t Lp = ((size_t)n + 2 * (size_t)(f.n_fft / 2) + 3) & ~(size_t)3;
  const size_t per = (Lp + (size_t)r->T * ((size_t)r->g_nfp + (size_t)r->g_nmp)) * sizeof(float);
  const size_t bc = sd_fb::FBG_CHUNK_BYTES / per < 1 ? 1 : sd_fb::FBG_CHUNK_BYTES / per;      // (per >= 4 Lp > 0)
  r->g_Lp = (int)Lp; r->g_Bc = (size_t)B < bc ? B : (int)bc;
  r->ws_need = ((size_t)r->g_Bc * per + 1023) & ~(size_t)255;
}

inline size_t sd_fbank_uniform_ws_bytes(const SdFbankFacts& f, int B, int n) {      // sd_fbank_workspace_bytes
  SdFbankRoute r = {};
  if (f.generic && B > 0 && n >= 0) sd_fbank_generic_layout(f, B, n, &r);
  return !f.generic ? sd_fbank_maxkey_bytes(B) : r.ws_need ? r.ws_need : 256;
}

// The route of a call sd_fbank_check accepts.  Uniform / lens / windows: the one-launch kernel where the switch is on, its tables exist,
// n <= U16_MAX_N and four samples lie behind `wav` (16-byte loads); else the folded kernel between the max-key fill and the finalize pass,
// tiles flat over (utterance, frame) from 32 frames on.  Packed: every span the route of a call for it alone (n_cap, n_lo).
inline SdFbankRoute sd_fbank_route(const SdFbankFacts& f, const SdFbankCall& c) {
  using namespace sd_fb;
  SdFbankRoute r = {};
  r.use_floor = f.log_mode == SD_LOG_DB_TOPDB && f.top_db >= 0.f;
  if (f.generic) {
    r.kinds = SD_FB_GENERIC;
    sd_fbank_generic_layout(f, c.B, c.n, &r);
    return r;
  }
  const bool packed = c.form == SD_FB_PACKED;
  const int longest = f.utt_switch && f.utt_tables ? U16_MAX_N : 0;
  r.T = frames(c.n);
  r.maxkey_bytes = r.tile_table_off = sd_fbank_maxkey_bytes(c.B);
  r.ws_need = packed ? sd_fbank_packed_ws_bytes(c.B) : r.maxkey_bytes;
  if (packed ? longest >= 1 : (c.n_total >= 4 && c.n <= longest)) {
    r.kinds |= SD_FB_ONE_LAUNCH;
    r.n_cap = c.n < longest ? c.n : longest;
    r.inv_row = recip32(f.n_mels % 4 == 0 ? f.n_mels / 4 : f.n_mels);
    r.utt16 = {c.B, U16_THREADS, u16_lds_bytes(r.n_cap)};      // (monotone in n: enough for every span of at most n_cap samples)
    if (!packed) return r;
  }
  r.n_lo = packed ? longest : 0;
  r.flat = !packed && r.T >= FOLD_FT;
  // a span of the folded route has at most T_s / 32 + 1 tiles: M / 32 + B in all (sd_fbank_check holds the bound to a grid whether or
  // not a span takes the route)
  r.tiles = packed ? (long)c.M / FOLD_FT + c.B : r.flat ? cdiv((long)c.B * r.T, FOLD_FT) : (long)c.B * cdiv(r.T, FOLD_FT);
  if (packed && c.n <= r.n_lo) return r;
  r.kinds |= SD_FB_FOLDED;
  r.inv_mels = recip32(f.n_mels);
  r.fill = {cdiv(c.B, 256), 256, 0};
  if (packed) r.tile_table = {1, 1024, 0};
  r.logmel = {cdiv(r.tiles, FOLD_WAVES), f.fold_threads, f.fold_lds};
  r.R = 320 / f.n_mels;
  if (r.R < 1) r.R = 1;
  if (!packed && r.R > r.T) r.R = r.T;                         // (a packed span's workgroup clamps R to its own T)
  r.finalize = {c.B, (int)cdiv((long)r.R * f.n_mels, 64) * 64, (size_t)r.R * f.n_mels * sizeof(float)};
  return r;
}

// Every argument refusal of the four entries, in the order the entries have always made them.  SD_OK: *r is the route (kinds 0: B = 0,
// nothing to do and nothing else looked at).  Otherwise the status code, with the text in why[SD_FB_WHY].
constexpr size_t SD_FB_WHY = 192;
#define SD_FB_NEED(code, cond, ...) do { if (!(cond)) { snprintf(why, SD_FB_WHY, __VA_ARGS__); return code; } } while (0)
inline int sd_fbank_check(const SdFbankFacts& f, const SdFbankCall& c, SdFbankRoute* r, char* why) {
  const char* const e = c.entry;
  const bool packed = c.form == SD_FB_PACKED;
  const int ARG = SD_ERR_ARG;
  *r = SdFbankRoute{};
  if (c.form == SD_FB_WINDOWS) {
    SD_FB_NEED(ARG, c.n_total >= 1, "%s: n_total=%lld", e, c.n_total);
    SD_FB_NEED(ARG, c.B == 0 || !c.no_starts, "%s: null starts", e);
  }
  SD_FB_NEED(ARG, !c.no_plan, "%s: null plan", e);
  if (packed) SD_FB_NEED(ARG, c.B >= 0, "%s: B=%d", e, c.B);
  else SD_FB_NEED(ARG, c.B >= 0 && c.n >= 0, "%s: B=%d n=%d", e, c.B, c.n);
  if (c.B == 0) return SD_OK;
  if (packed) {
    SD_FB_NEED(ARG, c.M > 0 && c.n >= 1, "%s: M=%d n_max=%d", e, c.M, c.n);
    SD_FB_NEED(ARG, !(c.no_wav || c.no_starts || c.no_lens || c.no_frame_start || c.no_out), "%s: null pointer", e);
    SD_FB_NEED(ARG, c.n_total >= 4, "%s: n_total=%lld (at least 4 samples)", e, c.n_total);
  } else {
    SD_FB_NEED(ARG, !c.no_wav && !c.no_out, "%s: null wav/out", e);
  }
  SD_FB_NEED(ARG, c.ld_out >= f.n_mels, "%s: ld_out=%d < n_mels=%d", e, c.ld_out, f.n_mels);
  // torch.stft(center=True, pad_mode="reflect") rejects n <= n_fft/2; zero padding needs one sample
  if (packed) SD_FB_NEED(SD_ERR_UNSUPPORTED, !f.generic && f.pad_mode == SD_PAD_ZERO, "%s: packed spans take the 25 ms / 10 ms plan with zero padding (speechbrain)", e);
  else if (f.pad_mode == SD_PAD_REFLECT)
    SD_FB_NEED(ARG, c.n > f.n_fft / 2, "%s: reflect padding of %d needs more than %d samples (got %d)", e, f.n_fft / 2, f.n_fft / 2, c.n);
  else SD_FB_NEED(ARG, c.n >= 1, "%s: empty waveform", e);
  if (f.generic) {
    const int T = sd_fbank_frames(f, c.n);
    SD_FB_NEED(ARG, T >= 1, "%s: %d samples give no frame at n_fft=%d", e, c.n, f.n_fft);
    SD_FB_NEED(ARG, (long long)T * c.B < (1LL << 31), "%s: too many frames", e);
  }
  *r = sd_fbank_route(f, c);
  if (f.generic) SD_FB_NEED(ARG, !c.ws_misaligned && c.ws_bytes >= r->ws_need, "%s: workspace too small or misaligned", e);
  else if (packed) SD_FB_NEED(ARG, !c.no_ws && c.ws_bytes >= r->ws_need && !c.ws_misaligned, "%s: workspace %zu < %zu bytes, or unaligned", e, c.ws_bytes, r->ws_need);
  else SD_FB_NEED(ARG, !c.no_ws && c.ws_bytes >= r->ws_need, "%s: workspace too small (%zu < %zu)", e, c.ws_bytes, r->ws_need);
  SD_FB_NEED(ARG, sd_fb::cdiv(r->tiles, sd_fb::FOLD_WAVES) < (1L << 31) && (!packed || r->tiles < (1L << 31)), "%s: grid too large", e);
  return SD_OK;
}
#undef SD_FB_NEED
