// Shared between sd_fbank.hip (plan, folded-DFT kernel, the four entries), sd_fbank_utt16.hip (the one-launch kernel with the factored DFT)
// and sd_fbank_generic.hip (any other framing).  What an entry refuses and which of the three runs, with what geometry: sd_fbank_route.h.
#pragma once
#include <cstring>
#include <initializer_list>

#include "sd_common.h"
#include "sd_fbank_route.h"

struct sd_fbank_plan {
  SdFbankFacts f;
  void* basis16_dev;       // folded-DFT kernel: f16 [pass][k step][tile][Chi | Clo | Shi | Slo][64][8]
  void* melw16_dev;        // folded-DFT kernel: bf16 [bin tile][k half][mel tile][W1 | W2][64][8]
  void* utt16_tables_dev;  // factored one-launch kernel (sd_fbank_utt16.hip): all of its fragment tables, 1 KB each
  // any other framing (sd_fbank_generic.hip): a float64 DFT kernel + the mel product on the exact-f32 conv operator
  void* g_wdft_dev;        // f64 [n_fft][2 nfp]: window[p] cos / -sin(2 pi k p / n_fft), (re, im) of a bin side by side
  void* g_wmel_dev;        // f32 [n_mels][1][nfp]
};

// whatever device tables the plan holds (a failed sd_fbank_plan_create, sd_fbank_plan_destroy)
inline void sd_fbank_free_tables(sd_fbank_plan* plan) {
  for (void** t : {&plan->basis16_dev, &plan->melw16_dev, &plan->utt16_tables_dev, &plan->g_wdft_dev, &plan->g_wmel_dev}) {
    if (*t) (void)hipFree(*t);
    *t = nullptr;
  }
}
// one device table from host memory; on failure the plan's tables are gone and the error is set
inline int sd_fbank_upload(sd_fbank_plan* plan, void** table, const void* host, size_t bytes) {
  hipError_t e = hipMalloc(table, bytes);
  if (e == hipSuccess) e = hipMemcpy(*table, host, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) return SD_OK;
  sd_fbank_free_tables(plan);
  return sd_set_error(SD_ERR_HIP, "sd_fbank_plan_create: device table upload failed: %s", hipGetErrorString(e));
}

// round-to-nearest-even f32 -> bf16 bits (finite inputs)
inline unsigned short sd_bf16_bits(float v) {
  unsigned u;
  std::memcpy(&u, &v, 4);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}
inline float sd_bf16_value(unsigned short b) {
  const unsigned u = (unsigned)b << 16;
  float v;
  std::memcpy(&v, &u, 4);
  return v;
}
// a table value as two f16 halves: hi = f16(v), lo = f16(v - hi)
inline void sd_split_f16(double v, _Float16* hi, _Float16* lo) {
  *hi = (_Float16)(float)v;
  *lo = (_Float16)(float)(v - (double)(float)*hi);
}

// the device pointers of a call (SdFbankCall says only which of them are null); lens != NULL: packed spans
struct SdFbankPtrs {
  const float* wav; const long long* starts; const int* lens; const int* frame_start; const float* rel_len;
  float* out; void* ws;
};

bool sd_fbank_generic_geometry_ok(int n_fft, int hop, int n_mels);
int sd_fbank_generic_create_tables(sd_fbank_plan* plan, const float* window, const float* mel_fb);
// what the route says, for the call (r, c) over the pointers p.  rel_len (device f32 [B] or NULL, with mean_norm): the per-bin mean over
// each row's first sd_norm_frames(rel_len[b], T) frames
int sd_fbank_generic_launch(const sd_fbank_plan* plan, const SdFbankRoute& r, const SdFbankCall& c, const SdFbankPtrs& p, hipStream_t stream);

// device tables of the factored kernel from the window (n_fft values) and the mel filterbank [n_fft / 2 + 1][n_mels]; it takes utterances
// of up to sd_fb::U16_MAX_N samples (the padded signal must fit the CU's LDS beside the table ring)
int sd_fbank_utt16_create_tables(sd_fbank_plan* plan, const float* window, const float* mel_fb);
// r.utt16: one workgroup per utterance of r.n_cap samples (uniform: c.n), or per packed span of at most so many
int sd_fbank_utt16_launch(const sd_fbank_plan* plan, const SdFbankRoute& r, const SdFbankCall& c, const SdFbankPtrs& p, hipStream_t stream);
