// ECAPA-TDNN forward on one HIP stream: the layer schedule behind
// EncoderClassifier.encode_batch [REF speech_encode.py:73-78] / ECAPAEncoder.forward
// [REF ecapa_annote.py:13-22], geometry per SURVEY.md Appendix A.3.
//
// Activations are [B*T][C], channel contiguous, resident in a caller-provided workspace for
// the whole forward (no allocation, no synchronisation here, so the call can be captured in a
// hipGraph).  Two precisions share this schedule:
//   f32  — exact f32 MFMA everywhere (sd_ecapa_forward_f32);
//   f16  — frame-level layers (M = B*T rows) take f16 weights / f16 activations with f32
//          accumulation; the per-segment layers (M = B rows: SE gate, global-context bias,
//          final FC) and all statistics stay f32 (sd_ecapa_forward_f16).
// Data movement avoided by construction:
//   * block outputs are written straight into their slice of the [B*T][3C] buffer the
//     MFA conv reads (no torch.cat copy);
//   * tdnn1 writes into the Res2Net result buffer, so chunk 0 needs no copy;
//   * the Res2Net add  c_{j+1} + y_j  is produced by the epilogue of conv j ("tee");
//   * the attention TDNN's global-context columns (mean/std broadcast over T) collapse
//     to a per-segment bias computed by one tiny GEMM.
//
// The file has three parts: the RULES, each routing condition as one function; make_plan(), a pure host
// function that turns them into the list of launches with the tensor forms each reads and writes (forms follow readers: a tensor
// exists in the forms its readers' routes ask for, and in no other); and run_step(), which launches one step as the plan states it.
// sd_ecapa_plan_read (sd_hip_trace.h) prints the same plan without a device.
#include <cstdlib>
#include <cstring>
#include <string>

#include "sd_common.h"
#include "sd_hip_trace.h"

namespace {

// ---------------------------------------------------------------- vocabulary (fixed in sd_hip_trace.h)
enum Buf : unsigned char { FEATS, X0, R, T2, XCAT, H, S0, S1, A1, E, XS, XCS, X0S, RS, WPK, SEMEAN, SEH, GATE, STATS, GBIAS, POOLED, SKP, EMB, N_BUF };
const char* const kBuf[N_BUF] = {"feats", "x0", "r", "t2", "xcat", "h", "s0", "s1", "a1", "e", "xs", "xcs", "x0s", "rs", "wpk", "semean", "seh", "gate",
                                 "stats", "gbias", "pooled", "skp", "emb"};
enum Form : unsigned char { NONE, AS_F32, AS_F16, AS_SPLIT, AS_STAT, AS_SCRATCH };     // AS_STAT: per-tile column sums of a conv epilogue
const char* const kForm[] = {"", "f32", "f16", "split", "stat", "scratch"};
enum Route : unsigned char { R_F32, R_SPLIT128, R_SPLIT128_FOLDED, R_SPLIT256_PACK, R_SPLIT256_TWIN, R_F16, R_PACKED, R_SEG_GEMM, R_CHAIN, R_CAST,
                             R_PACK, R_ASP_FUSED, R_ASP_POOL, R_SE_SCALE, R_COLSTAT_FINISH, R_SEG_MEAN_STD };
const char* const kRoute[] = {"f32", "split128", "split128_folded", "split256_pack", "split256_twin", "f16", "packed", "seg_gemm", "chain", "cast",
                              "pack", "asp_fused", "asp_pool", "se_scale", "colstat_finish", "seg_mean_std"};
enum Op : unsigned char { OP_CAST, OP_PACK, OP_STEM, OP_TDNN1, OP_RES2, OP_CHAIN, OP_TDNN2, OP_SQUEEZE, OP_SE1, OP_SE2, OP_SCALE, OP_MFA, OP_STATS,
                          OP_ASP_G, OP_ASP_H, OP_ASP_CONV, OP_POOL, OP_FC };
const char* const kOp[] = {"cast", "pack", "stem", "tdnn1", "res2", "chain", "tdnn2", "squeeze", "se1", "se2", "scale", "mfa", "stats",
                           "asp_g", "asp_h", "asp_conv", "pool", "fc"};

struct TRef { unsigned char buf, form; int ld, col0, cols; };      // columns [col0, col0 + cols) of rows of ld VALUE columns; form NONE: absent
// One launch.  A conv: rd = {x, tee_add source, per-segment bias}, wr = {y, tee, column statistics}.  se_scale: rd = {t2, shortcut, gate},
// wr = {the f32 / f16 slice, its SD_DT_SPLIT16 twin}.  A finish pass: rd = {y, its column statistics}.  j: the Res2Net step; of a pack
// step, the Op it feeds.
struct Step { unsigned char op, route; signed char blk, j; TRef rd[3], wr[3]; };
constexpr int kMaxSteps = 2 + SD_MAX_BLOCKS * (9 + SD_MAX_RES2) + 8;
struct Plan { int n; const char* bad; Step s[kMaxSteps]; };
struct Tensor { TRef plain, twin; };                                // the forms one activation tensor exists in: f32 / f16, SD_DT_SPLIT16

// The four A/B switches for measurements (=0 turns a route off), read once per process behind sd_experiment_env
struct Switches { bool colstat, stem_cast, res2_fused, asp_fused; };
const Switches& switches() {
  static const Switches s = [] {
    auto on = [](const char* name) { const char* e = sd_experiment_env(name); return !(e && e[0] == '0'); };
    return Switches{on("SD_COLSTAT"), on("SD_STEM_CAST"), on("SD_RES2_FUSED"), on("SD_ASP_FUSED")};
  }();
  return s;
}

// split16 = 1, "f32-split16x3": every frame-level contraction on the f16 matrix cores, three products per value pair, f32-level accuracy;
// split16 = 2: only the narrow layers (Res2Net convs, attention TDNN, the attention logits of the pooling kernel); the wide layers,
// 86 % of the flops, stay on the exact-f32 kernel
bool any_split(const sd_ecapa_weights* w, int dt) { return w->split16 != 0 && dt == SD_DT_F32; }
bool wide_split(const sd_ecapa_weights* w, int dt) { return w->split16 == 1 && dt == SD_DT_F32; }

enum { MAP_UNIFORM, MAP_LENGTHS, MAP_PACKED };
// tune: the tuning snapshot (sd_conv_choice.h), taken ONCE per forward: the plan decides up front which tensors exist only as
// SD_DT_SPLIT16, so every rule and every conv of one forward must see the same values whatever sd_set_tuning() does meanwhile.
struct PlanIn {
  const sd_ecapa_weights* w; int B, T, M, map, dt; SdConvTuning tune; Switches sw; bool feats_aligned;
  long narrow_tiles() const { return tune.tune[SD_TUNE_F16_NARROW_TILES]; }
  int Tc() const { return map == MAP_PACKED ? M : T; }            // the segment length the position-free layers see
  bool split() const { return any_split(w, dt); }
  bool wsplit() const { return wide_split(w, dt); }
};

// ---------------------------------------------------------------- rules: each condition once
// Which optional buffers a geometry and mode have -- never B, M or the tuning: a caller sizes one workspace for its largest micro-batch
// and runs a shorter one in it.  xs: pack scratch of a wide conv's input; xcs: SD_DT_SPLIT16 twin of xcat, written by the SE scale +
// residual kernel; x0s: the stem's output as SD_DT_SPLIT16; rs: the Res2Net output r as SD_DT_SPLIT16, written by the narrow convs;
// wpk: Res2Net chain weights in fragment order (f16).
bool has_buf(const sd_ecapa_weights* w, int dt, int buf) {
  const int C = w->channels, Cm = w->mfa_channels;
  const bool wsplit = wide_split(w, dt);
  switch (buf) {
    case XS: return wsplit;
    case XCS: return wsplit && Cm % 32 == 0 && C % 32 == 0;
    case X0S: return wsplit && C % 32 == 0;
    case RS: return wsplit && C % 32 == 0 && (C / w->res2_scale) % 32 == 0;
    case WPK: return dt == SD_DT_F16;
    default: return true;
  }
}

// Small launches of the C-wide layers go to the narrow split kernel, which has no column statistics: sd_wide_goes_narrow (sd_conv_choice.h)
bool wide_goes_narrow(const PlanIn& in, const sd_layer& l) { return sd_wide_goes_narrow(l.cout, in.M, in.narrow_tiles()); }

// The wide kernel's packing: weights scaled by 2^s with the scale folded into bias_split / scale_split.  A wide-ROLE layer (stem,
// tdnn1, tdnn2, MFA) of a small geometry (cout <= 256) may carry the NARROW packing instead (w_split + split_scale_inv, no folded
// vectors): it then runs on the 128x128 split kernel with its own bias / scale, or on the exact kernel.
bool wide_packed(const sd_layer& l) { return l.w_split && l.bias_split && l.scale_split; }

// The SE squeeze / the pooling's global mean and std come out of a wide conv's epilogue as per-tile column sums, parked in `scratch`
// bytes of a dead buffer, where the geometry allows.  The epilogue sums over all T rows of a segment: uniform map only.  The buffers are
// sized for the smallest row unit a launch can write: an f32 forward can reach the exact operator's 80 / 96 / 112-row tiles
// (SD_CONV_OP_F32_STAT_ROWS) also WITH split weights; the f16 and split kernels always write units of 128.  The floor on T is the
// operator's own (SdConvRule::colstat_T).
bool colstat_rule(const PlanIn& in, const sd_layer& l, size_t scratch) {
  const size_t unit = in.dt == SD_DT_F32 ? SD_STAT_UNIT_MIN : SD_T128;
  return in.sw.colstat && in.map == MAP_UNIFORM && in.T >= (in.wsplit() ? SD_COLSTAT_T_256 : SD_COLSTAT_T_128) && l.cout % 256 == 0 &&
         !(in.wsplit() && l.w_split && wide_goes_narrow(in, l)) && (size_t)((in.M + unit - 1) / unit) * 6 * l.cout * sizeof(float) <= scratch;
}

// what the 128x128 split kernel needs of the f32 operand it splits while staging
bool stage_aligned(const sd_layer& l, int ld, int col0) { return l.cin % 4 == 0 && ld % 4 == 0 && col0 % 4 == 0; }

// A wide layer of the f32 schedule: in split16 mode (and when the layer carries the second packing) it runs on the f16 matrix cores
// with three products per value pair, on the 256x256 kernel over an SD_DT_SPLIT16 input (R_SPLIT256_PACK here; make_plan turns it into
// R_SPLIT256_TWIN where the producer writes that form) or, a small launch, on the 128x128 kernel; otherwise the exact-f32 kernel.
Route wide_route(const PlanIn& in, const sd_layer& l, int ld, int col0, bool colstat) {
  if (in.dt == SD_DT_F16) return R_F16;
  if (in.wsplit() && l.w_split && !wide_packed(l))
    // narrow packing on a wide-role layer: the weights are scaled by 2^s and NOTHING else carries the scale, so the only split
    // kernel that may take them is the 128x128 one with w_scale_inv (the layer's own bias / scale); otherwise exact f32
    return l.split_scale_inv > 0.f && !colstat && stage_aligned(l, ld, col0) ? R_SPLIT128 : R_F32;
  if (!(in.wsplit() && wide_packed(l))) return R_F32;
  // (f32 x stays: split while staged; the folded 2^s form of bias / scale serves this kernel too.  Column statistics have yielded to a
  // small launch in colstat_rule, and start at T = 128 there, which is what the 256x256 kernel needs of them)
  return wide_goes_narrow(in, l) && stage_aligned(l, ld, col0) ? R_SPLIT128_FOLDED : R_SPLIT256_PACK;
}

// Does a layer on `route` read the SD_DT_SPLIT16 twin of its input (buffer `twin`, same layout as the f32 buffer) instead of packing it?
bool reads_twin(const PlanIn& in, Route route, const sd_layer& l, int twin, int col0) {
  return route == R_SPLIT256_PACK && has_buf(in.w, in.dt, twin) && l.cin % 32 == 0 && col0 % 32 == 0;
}

// A narrow layer of the f32 schedule (Res2Net convs, attention TDNN): in split16 mode, when it carries the second packing, the
// 128x128 split kernel (f32 activations split while staged; tee / tee_add / per-segment bias as in the exact kernel).
// Small launches (at most 56 tiles of 128x128: up to ~35 two-second segments) stay on the exact-f32 operator, whose ring kernel spreads
// them over 64x64 / 32x64 tiles: measured per launch at 16 / 32 segments, Res2Net conv 9.5 / 14.3 us exact against 17.7 / 19.0 split (26 / 51
// workgroups of 128x128), attention TDNN 49 / 76 against 105 / 110; at 64 segments the split kernel is ahead again.  The exact operator
// cannot write SD_DT_SPLIT16: a launch whose reader wants that form is not small.
Route narrow_route(const PlanIn& in, const sd_layer& l, bool y_split) {
  if (in.dt == SD_DT_F16) return R_F16;
  const long tiles128 = (long)((in.M + 127) / 128) * ((l.cout + 127) / 128);
  const bool small = in.Tc() > 1 && tiles128 <= 56 && !y_split;
  return !small && in.split() && l.w_split && !l.bias_split ? R_SPLIT128 : R_F32;
}

// A position-dependent layer (the k = 5 stem, the dilated Res2Net convs, the attention TDNN with its per-segment bias): packed spans take
// the packed conv (reflect and bias per span), a uniform map the layer's own route.
Route positional(const PlanIn& in, Route uniform) { return in.map == MAP_PACKED ? R_PACKED : uniform; }

// ---------------------------------------------------------------- the plan
TRef ref(int buf, int form, int ld, int col0, int cols) { return TRef{(unsigned char)buf, (unsigned char)form, ld, col0, cols}; }
TRef all(int buf, int form, int cols) { return ref(buf, form, cols, 0, cols); }      // every column of rows of `cols`

Step& add(Plan* p, Op op, Route route, int blk, int j, const TRef& rd0, const TRef& wr0) {
  Step& s = p->s[p->n++];
  s = Step{};
  s.op = op; s.route = route; s.blk = (signed char)blk; s.j = (signed char)j;
  s.rd[0] = rd0; s.wr[0] = wr0;
  return s;
}

// A wide-role layer on its route: the 256x256 split kernel reads the twin where one exists, else a pack pass re-writes the f32 input
// as SD_DT_SPLIT16 rows in xs (4 bytes per value in, 4 out).  The one defensive refusal: a form no step writes.
Step& add_wide(Plan* p, const PlanIn& in, Op op, int blk, const sd_layer& l, Route route, const Tensor& x, const TRef& y) {
  TRef src = x.plain;
  if (route == R_SPLIT256_PACK && x.twin.form && reads_twin(in, route, l, x.twin.buf, x.twin.col0)) {
    route = R_SPLIT256_TWIN;
    src = x.twin;
  } else if (route == R_SPLIT256_PACK && src.form) {
    const TRef xs = all(XS, AS_SPLIT, (l.cin + 31) / 32 * 32);
    add(p, OP_PACK, R_PACK, blk, op, ref(src.buf, src.form, src.ld, src.col0, l.cin), xs);
    src = xs;
  }
  if (!src.form) p->bad = kOp[op];
  return add(p, op, route, blk, -1, src, y);
}

// the statistics of a conv's output y: from its column statistics where the conv wrote them, else from a pass over y
void add_finish(Plan* p, Op op, int blk, const Step& conv, const TRef& out) {
  add(p, op, conv.wr[2].form ? R_COLSTAT_FINISH : R_SEG_MEAN_STD, blk, -1, conv.wr[0], out).rd[1] = conv.wr[2];
}

// Relative lengths (map MAP_LENGTHS, speechbrain's wav_lens): every conv, BN, Res2Net add and the SE gate's application run on the padded
// rows as without them; the SE squeezes, the global mean / std of the attentive pooling and its softmax and statistics count each row's
// first sd_mask_frames(rel_len[b], T) frames only.  Those statistics then come from the reduction kernels (no column statistics from the
// conv epilogues), and both pooling routes take the mask.
// Packed spans ("Packed spans", sd_hip.h; exact f32 only): the position-dependent layers run on the packed conv, the position-free 1x1
// layers on the uniform operator as ONE segment of M rows (T = M: the reflect is a no-op), every statistic and the SE gate on the packed
// map; the per-segment layers (B rows) as always.
int make_plan(const PlanIn& in, Plan* p) {
  const sd_ecapa_weights* w = in.w;
  const int C = w->channels, Cm = w->mfa_channels, chunk = C / w->res2_scale, att = w->att_channels, nm = w->n_mels, n = w->n_blocks, sc = w->res2_scale;
  const int A = in.dt == SD_DT_F16 ? AS_F16 : AS_F32;
  const size_t es = in.dt == SD_DT_F16 ? 2 : 4;
  const TRef none = {};
  p->n = 0; p->bad = nullptr;
  // The readers that decide a tensor's form.  Slice i of xcat (block i's output) is read by the MFA conv, by the next block's tdnn1 and by
  // the next block's shortcut; the shortcut takes whichever form the other two leave (f32 first).  With the wide layers split all three
  // take the twin, so the f32 slice is not written -- unless a small launch routes the next tdnn1 to the narrow kernel, which stages f32.
  const bool mfa_stat = colstat_rule(in, w->mfa, (size_t)in.M * C * es);         // (column sums in r, dead since the last block's tdnn2)
  const Route mfa_route = wide_route(in, w->mfa, Cm, 0, mfa_stat);
  const bool mfa_twin = reads_twin(in, mfa_route, w->mfa, XCS, 0);
  Route t1_route[SD_MAX_BLOCKS];
  bool t1_twin[SD_MAX_BLOCKS];                                                    // tdnn1 of block i reads x0 (i = 0) or slice i - 1
  for (int i = 0; i < n; ++i) {
    t1_route[i] = wide_route(in, w->blocks[i].tdnn1, i ? Cm : C, i ? (i - 1) * C : 0, false);
    t1_twin[i] = reads_twin(in, t1_route[i], w->blocks[i].tdnn1, i ? XCS : X0S, i ? (i - 1) * C : 0);
  }
  auto slice_twin = [&](int i) { return mfa_twin || (i + 1 < n && t1_twin[i + 1]); };
  auto slice_plain = [&](int i) { return !mfa_twin || (i + 1 < n && !t1_twin[i + 1]); };

  // block 0: TDNNBlock(n_mels -> C, k=5) on the f32 features.  f16: the features are rounded to f16 once (the operand precision of
  // that path anyway; t2 is free here), which lets the stem run on the LDS-DMA kernel of the wide layers (-0.75 ms per 5000 segments:
  // 106.6 -> 108.3 k segments/s).
  // The stem writes SD_DT_SPLIT16 and nothing else (no f32 tensor, no pack pass) iff it can (the 256x256 split kernel) and both readers
  // take that form: block 1's tdnn1, and its shortcut, whose kernel reads a split shortcut only while it writes a twin itself.
  Tensor x;
  {
    TRef f = all(FEATS, AS_F32, nm);
    if (in.dt == SD_DT_F16 && in.sw.stem_cast && ((long)in.M * nm) % 8 == 0 && in.feats_aligned) f = add(p, OP_CAST, R_CAST, -1, -1, f, all(T2, AS_F16, nm)).wr[0];
    const Route route = wide_route(in, w->block0, nm, 0, false);
    const bool split_only = route == R_SPLIT256_PACK && t1_twin[0] && slice_twin(0);
    x.plain = split_only ? none : all(X0, A, C);
    x.twin = split_only ? all(X0S, AS_SPLIT, C) : none;
    add_wide(p, in, OP_STEM, -1, w->block0, positional(in, route), Tensor{f, none}, split_only ? x.twin : x.plain);
  }
  for (int i = 0; i < n; ++i) {
    const sd_se_res2_block& blk = w->blocks[i];
    // Res2Net chain: y_j = TDNN_j(c_j + y_{j-1}), written over chunk j of r.  f16: one kernel per block keeps the
    // segment's chain state in LDS (sd_res2net_f16.hip); otherwise (f32, or a segment too long for LDS) one conv per
    // step, chunk 1 teed to s0 by tdnn1 and the adds c_{j+1} + y_j produced by each conv's epilogue.
    const bool chain = in.sw.res2_fused && in.dt == SD_DT_F16 && sc >= 2 && sd_res2net_chain_supported(in.T, chunk, sc - 1, blk.res2[0].taps, blk.res2[0].dil);
    // tdnn2; the SE squeeze (mean over T) comes out of its epilogue where the geometry allows (the Res2Net scratch s0 is dead and holds
    // the sums), else from a pass over t2
    const bool stat = colstat_rule(in, blk.tdnn2, (size_t)in.M * chunk * es);
    const Route t2_route = wide_route(in, blk.tdnn2, C, 0, stat);
    // tdnn2 reads r as SD_DT_SPLIT16 iff every narrow conv can write its chunk in that form directly (same bytes as the f32 chunk, no
    // pack pass: 8 of the pass's 8 bytes per value go); only chunk 0, which tdnn1's output passes through unchanged, is packed, and r
    // itself keeps tdnn1's output (the tee_add source of every conv)
    bool r_twin = !chain && reads_twin(in, t2_route, blk.tdnn2, RS, 0);
    for (int j = 1; j < sc && r_twin; ++j) r_twin = blk.res2[j - 1].w_split != nullptr && !blk.res2[j - 1].bias_split;

    Step& t1 = add_wide(p, in, OP_TDNN1, i, blk.tdnn1, t1_route[i], x, all(R, A, C));
    if (chain) {
      add(p, OP_CHAIN, R_CHAIN, i, -1, all(R, A, C), ref(R, A, C, chunk, C - chunk)).wr[1] = all(WPK, AS_SCRATCH, 0);
    } else {
      t1.wr[1] = all(S0, A, chunk);
      if (r_twin) add(p, OP_PACK, R_PACK, i, OP_TDNN2, ref(R, A, C, 0, chunk), ref(RS, AS_SPLIT, C, 0, chunk));
      for (int j = 1; j < sc; ++j) {
        const Route route = positional(in, narrow_route(in, blk.res2[j - 1], r_twin));
        if (r_twin && route != R_SPLIT128) p->bad = kOp[OP_RES2];
        Step& s = add(p, OP_RES2, route, i, j, all((j & 1) ? S0 : S1, A, chunk), ref(r_twin ? RS : R, r_twin ? AS_SPLIT : A, C, j * chunk, chunk));
        if (j + 1 < sc) { s.rd[1] = ref(R, A, C, (j + 1) * chunk, chunk); s.wr[1] = all((j & 1) ? S1 : S0, A, chunk); }
      }
    }
    Step& t2 = add_wide(p, in, OP_TDNN2, i, blk.tdnn2, t2_route, Tensor{r_twin ? none : all(R, A, C), r_twin ? all(RS, AS_SPLIT, C) : none}, all(T2, A, C));
    if (stat) t2.wr[2] = all(S0, AS_STAT, C);
    add_finish(p, OP_SQUEEZE, i, t2, all(SEMEAN, AS_F32, C));
    // squeeze-excitation gate (per-segment, f32)
    Step& se1 = add(p, OP_SE1, R_SEG_GEMM, i, -1, all(SEMEAN, AS_F32, C), all(SEH, AS_F32, blk.se1.cout));
    Step& se2 = add(p, OP_SE2, R_F32, i, -1, se1.wr[0], all(GATE, AS_F32, C));
    // gate * t2 + shortcut -> slice i of the MFA input, in the forms its readers take
    Step& s = add(p, OP_SCALE, R_SE_SCALE, i, -1, t2.wr[0], none);
    s.rd[1] = x.plain.form ? x.plain : x.twin; s.rd[2] = se2.wr[0];
    x.plain = s.wr[0] = slice_plain(i) ? ref(XCAT, A, Cm, i * C, C) : none;
    x.twin = s.wr[1] = slice_twin(i) ? ref(XCS, AS_SPLIT, Cm, i * C, C) : none;
    if (s.rd[1].form == AS_SPLIT && !x.twin.form) p->bad = kOp[OP_SCALE];
  }
  // multi-layer feature aggregation; the global mean / std of attentive pooling likewise from the epilogue
  Step& m = add_wide(p, in, OP_MFA, -1, w->mfa, mfa_route, Tensor{mfa_twin ? none : all(XCAT, A, Cm), mfa_twin ? all(XCS, AS_SPLIT, Cm) : none}, all(H, A, Cm));
  if (mfa_stat) m.wr[2] = all(R, AS_STAT, Cm);
  add_finish(p, OP_STATS, -1, m, all(STATS, AS_F32, 2 * Cm));
  // attentive statistics pooling with global context
  Step& g = add(p, OP_ASP_G, R_SEG_GEMM, -1, -1, all(STATS, AS_F32, 2 * Cm), all(GBIAS, AS_F32, att));
  Step& h = add(p, OP_ASP_H, positional(in, narrow_route(in, w->asp_tdnn_h, false)), -1, -1, m.wr[0], all(A1, A, att));
  h.rd[2] = g.wr[0];
  // asp.conv + softmax over T + weighted statistics: one kernel where the geometry allows (the [M][3C] logits are then never
  // stored), else the conv followed by the pooling kernel
  const TRef pooled = all(POOLED, AS_F32, 2 * Cm);
  if (in.sw.asp_fused && in.map != MAP_PACKED && w->asp_conv.taps == 1 && w->asp_conv.cin_pad == att && sd_asp_attend_pool_supported(in.dt, in.T, Cm, att)) {
    add(p, OP_POOL, R_ASP_FUSED, -1, -1, h.wr[0], pooled).rd[1] = m.wr[0];
  } else {
    Step& c = add(p, OP_ASP_CONV, in.dt == SD_DT_F16 ? R_F16 : R_F32, -1, -1, h.wr[0], all(E, A, Cm));
    add(p, OP_POOL, R_ASP_POOL, -1, -1, c.wr[0], pooled).rd[1] = m.wr[0];
  }
  // asp_bn (folded into the weights by the host) + fc
  add(p, OP_FC, R_SEG_GEMM, -1, -1, pooled, all(EMB, AS_F32, w->emb_dim));
  if (p->bad) return sd_set_error(SD_ERR_UNSUPPORTED, "sd_ecapa_forward: step %s reads or writes a tensor form the plan does not hold", p->bad);
  return SD_OK;
}

// ---------------------------------------------------------------- workspace
struct Carver {
  char* base; size_t off;
  void* take(size_t elems, size_t esz) {          // base == nullptr: a sizing pass (no pointer is formed from a null base)
    void* p = base ? base + off : nullptr;
    off += (elems * esz + 255) & ~(size_t)255;
    return p;
  }
};

struct Buffers {
  void* p[N_BUF];     // x0 .. e: activation dtype (e = attention logits); xs .. wpk: see has_buf; semean .. pooled: f32 per segment
  size_t wpk_bytes;
  size_t skp_bytes;   // skp: partial sums of the per-segment layers' grid split-K (sd_seg_gemm_f32)
  size_t bytes;
};

int max_i(int a, int b) { return a > b ? a : b; }

// M: activation rows (B * T; packed spans: the total of their frames)
Buffers carve(const sd_ecapa_weights* w, int B, size_t M, void* ws, int act_dtype) {
  const size_t es = act_dtype == SD_DT_F16 ? 2 : 4;
  const int C = w->channels, Cm = w->mfa_channels, chunk = C / w->res2_scale;
  int se = 0;
  for (int i = 0; i < w->n_blocks; ++i) se = max_i(se, w->blocks[i].se1.cout);
  Carver c{static_cast<char*>(ws), 0};
  Buffers b = {};
  auto take = [&](int buf, size_t elems, size_t esz) { b.p[buf] = has_buf(w, act_dtype, buf) ? c.take(elems, esz) : nullptr; };
  take(X0, M * max_i(C, w->att_channels), es);
  take(R, M * C, es);
  take(T2, M * C, es);
  // the concatenated block outputs are dead after the MFA conv; the attention logits reuse the space
  take(XCAT, M * Cm, es);
  take(H, M * Cm, es);
  take(S0, M * chunk, es);
  take(S1, M * chunk, es);
  take(SEMEAN, (size_t)B * C, 4);
  take(SEH, (size_t)B * se, 4);
  take(GATE, (size_t)B * C, 4);
  take(STATS, (size_t)B * 2 * Cm, 4);
  take(GBIAS, (size_t)B * w->att_channels, 4);
  take(POOLED, (size_t)B * 2 * Cm, 4);
  // scratch of the grid split-K (M <= 256 rows): the largest of the three per-segment layers that use it (final FC at B = 256: 4.7 MB).
  // Above 256 rows the layers take the plain operator and the scratch is idle, but its 256-row share stays reserved: a caller sizes one
  // workspace for its largest micro-batch and runs a shorter last one in it, so the size must never shrink as B grows (it dropped by
  // this share from B = 256 to 257, and a workspace sized for 257 .. 286 rows refused the <= 256-row remainder with SD_ERR_WORKSPACE)
  {
    const int Bs = B < 256 ? B : 256;
    size_t need = sd_seg_gemm_scratch_bytes(Bs, w->fc.cin_pad, w->fc.cout);
    const size_t g = sd_seg_gemm_scratch_bytes(Bs, w->asp_tdnn_g.cin_pad, w->asp_tdnn_g.cout);
    need = g > need ? g : need;
    for (int i = 0; i < w->n_blocks; ++i) {
      const size_t s1 = sd_seg_gemm_scratch_bytes(Bs, w->blocks[i].se1.cin_pad, w->blocks[i].se1.cout);
      need = s1 > need ? s1 : need;
    }
    b.skp_bytes = (need + 255) & ~(size_t)255;
  }
  take(SKP, b.skp_bytes, 1);
  if (!b.skp_bytes) b.p[SKP] = nullptr;
  b.wpk_bytes = has_buf(w, act_dtype, WPK) ? sd_res2net_chain_workspace_bytes(w->res2_scale - 1) : 0;
  take(WPK, b.wpk_bytes, 1);
  take(XS, M * (size_t)((Cm + 31) / 32 * 32), 4);
  take(XCS, M * (size_t)Cm, 4);
  take(X0S, M * (size_t)C, 4);
  take(RS, M * (size_t)C, 4);
  b.p[A1] = b.p[X0];    // block-0 output is dead once block 1 has consumed it
  b.p[E] = b.p[XCAT];
  b.bytes = c.off;
  return b;
}

int check_layer(const char* name, const sd_layer& l, int cin, int cout, int taps, int dtype) {
  SD_CHECK_ARG(l.w != nullptr, "sd_ecapa: layer %s has no weights", name);
  SD_CHECK_ARG(l.cin == cin && l.cout == cout && l.taps == taps,
               "sd_ecapa: layer %s is %d->%d k=%d, geometry wants %d->%d k=%d", name, l.cin, l.cout, l.taps, cin, cout, taps);
  SD_CHECK_ARG(l.w_dtype == dtype, "sd_ecapa: layer %s weights are dtype %d, schedule wants %d", name, l.w_dtype, dtype);
  return SD_OK;
}

int check_weights(const sd_ecapa_weights* w, int act_dtype) {
  SD_CHECK_ARG(w != nullptr, "sd_ecapa: null weights");
  SD_CHECK_ARG(w->w_dtype == act_dtype, "sd_ecapa: weights were packed for dtype %d, forward is dtype %d", w->w_dtype, act_dtype);
  SD_CHECK_ARG(w->n_blocks >= 1 && w->n_blocks <= SD_MAX_BLOCKS, "sd_ecapa: n_blocks=%d", w->n_blocks);
  SD_CHECK_ARG(w->res2_scale >= 2 && w->res2_scale - 1 <= SD_MAX_RES2, "sd_ecapa: res2_scale=%d", w->res2_scale);
  const int gran = act_dtype == SD_DT_F16 ? 8 : 4;
  SD_CHECK_ARG(w->channels % (gran * w->res2_scale) == 0, "sd_ecapa: channels=%d must be a multiple of %d*res2_scale", w->channels, gran);
  SD_CHECK_ARG(w->mfa_channels == w->n_blocks * w->channels, "sd_ecapa: mfa_channels=%d != n_blocks*channels", w->mfa_channels);
  SD_CHECK_ARG(w->n_mels % gran == 0 && w->att_channels % gran == 0, "sd_ecapa: n_mels / att_channels must be multiples of %d", gran);
  const int C = w->channels, Cm = w->mfa_channels, chunk = C / w->res2_scale;
  const int fd = act_dtype;       // frame-level layers
  const int sd = SD_DT_F32;       // per-segment layers
  if (int e = check_layer("block0", w->block0, w->n_mels, C, w->block0.taps, fd)) return e;
  for (int i = 0; i < w->n_blocks; ++i) {
    const sd_se_res2_block& b = w->blocks[i];
    if (int e = check_layer("tdnn1", b.tdnn1, C, C, 1, fd)) return e;
    for (int j = 0; j < w->res2_scale - 1; ++j)
      if (int e = check_layer("res2net", b.res2[j], chunk, chunk, b.res2[j].taps, fd)) return e;
    if (int e = check_layer("tdnn2", b.tdnn2, C, C, 1, fd)) return e;
    if (int e = check_layer("se1", b.se1, C, b.se1.cout, 1, sd)) return e;
    if (int e = check_layer("se2", b.se2, b.se1.cout, C, 1, sd)) return e;
    SD_CHECK_ARG(b.se1.cout % 4 == 0, "sd_ecapa: se_channels must be a multiple of 4");
  }
  if (int e = check_layer("mfa", w->mfa, Cm, Cm, 1, fd)) return e;
  if (int e = check_layer("asp_tdnn_h", w->asp_tdnn_h, Cm, w->att_channels, 1, fd)) return e;
  if (int e = check_layer("asp_tdnn_g", w->asp_tdnn_g, 2 * Cm, w->att_channels, 1, sd)) return e;
  if (int e = check_layer("asp_conv", w->asp_conv, w->att_channels, Cm, 1, fd)) return e;
  if (int e = check_layer("fc", w->fc, 2 * Cm, w->emb_dim, 1, sd)) return e;
  return SD_OK;
}

int check_packed_weights(const sd_ecapa_weights* w) {
  if (w->w_dtype != SD_DT_F32 || w->split16 != 0)
    return sd_set_error(SD_ERR_UNSUPPORTED, "sd_ecapa_forward_packed_f32: packed spans run the exact-f32 schedule only (weights: dtype %d, split16 %d)",
                        w->w_dtype, w->split16);
  return SD_OK;
}

// ---------------------------------------------------------------- the executor: one step, as the plan states it
sd_conv_args conv_of(const sd_layer& l, const void* x, int x_dtype, int lda, int a_col0, void* y, int y_dtype, int ldo, int o_col0,
                     int M, int T, int act) {
  sd_conv_args a = {};
  a.x = x; a.lda = lda; a.a_col0 = a_col0; a.x_dtype = x_dtype;
  a.w = l.w; a.w_dtype = l.w_dtype;
  a.y = y; a.ldo = ldo; a.o_col0 = o_col0; a.y_dtype = y_dtype;
  a.M = M; a.T = T;
  a.cin = l.cin; a.cin_pad = l.cin_pad; a.cout = l.cout; a.taps = l.taps; a.dil = l.dil;
  a.bias = l.bias; a.bias_per_seg = 0;
  a.act = act; a.scale = l.scale; a.shift = l.shift; a.act2 = SD_ACT_NONE;
  return a;
}

const sd_layer& layer_of(const sd_ecapa_weights* w, const Step& s) {
  switch (s.op) {
    case OP_STEM: return w->block0;
    case OP_TDNN1: return w->blocks[s.blk].tdnn1;
    case OP_RES2: return w->blocks[s.blk].res2[s.j - 1];
    case OP_TDNN2: case OP_SQUEEZE: return w->blocks[s.blk].tdnn2;
    case OP_SE1: return w->blocks[s.blk].se1;
    case OP_SE2: return w->blocks[s.blk].se2;
    case OP_MFA: case OP_STATS: return w->mfa;
    case OP_ASP_G: return w->asp_tdnn_g;
    case OP_ASP_H: return w->asp_tdnn_h;
    case OP_ASP_CONV: return w->asp_conv;
    default: return w->fc;
  }
}

int dtype_of(int form) { return form == AS_F16 ? SD_DT_F16 : form == AS_SPLIT ? SD_DT_SPLIT16 : SD_DT_F32; }

struct Exec { const sd_ecapa_weights* w; const SdSegs& sg; const Buffers& b; sd_stream_t stream; int M, Tc, dt; bool split; const SdConvTuning& tune; };

// stat_rows: the row unit of the column statistics the last conv wrote (128 unless the exact-f32 operator picked one of its 80 / 96 /
// 112-row tiles: small launches), for the finish pass that follows it
int run_step(const Exec& x, const Step& s, int* stat_rows) {
  const sd_ecapa_weights* w = x.w;
  void* const* p = x.b.p;
  const int B = x.sg.B, T = x.sg.T, C = w->channels, Cm = w->mfa_channels, chunk = C / w->res2_scale;
  const sd_layer& l = layer_of(w, s);
  const TRef &x0 = s.rd[0], &x1 = s.rd[1], &y0 = s.wr[0];
  const int pool = s.op == OP_STATS;       // the pooling's statistics want the std too
  switch (s.route) {
    case R_CAST: return sd_cast_f32_f16(static_cast<const float*>(p[x0.buf]), (long)x.M * x0.cols, p[y0.buf], x.stream);
    case R_PACK: return sd_split16_pack_f32(static_cast<const float*>(p[x0.buf]), x0.ld, x0.col0, x.M, x0.cols, 1.f, p[y0.buf], y0.ld, x.stream);
    case R_CHAIN: return sd_res2net_chain_f16(p[R], C, B, T, w->blocks[s.blk].res2, w->res2_scale - 1, p[WPK], x.b.wpk_bytes, x.stream);
    case R_COLSTAT_FINISH:
      return sd_colstat_finish_rows(static_cast<float*>(p[x1.buf]), l.shift, p[x0.buf], x.dt, x0.ld, 0, B, T, x0.cols, pool, pool ? w->asp_eps : 0.f,
                                    static_cast<float*>(p[y0.buf]), *stat_rows, x.stream);
    case R_SEG_MEAN_STD:
      return sd_seg_mean_std(p[x0.buf], x.dt, x0.ld, 0, x.sg, x0.cols, pool, pool ? w->asp_eps : 0.f, static_cast<float*>(p[y0.buf]), x.stream);
    case R_SE_SCALE: {     // (a split shortcut has the layout of its f32 buffer, whose pointer the kernel still wants)
      const int plain = x1.buf == X0S ? X0 : x1.buf == XCS ? XCAT : x1.buf;
      return sd_se_scale_residual(p[T2], C, static_cast<float*>(p[GATE]), p[plain], x1.ld, x1.col0, p[XCAT], Cm, s.blk * C, x.sg, C, x.dt, x.stream,
                                  s.wr[1].form ? p[XCS] : nullptr, Cm, s.blk * C, x1.form == AS_SPLIT ? p[x1.buf] : nullptr, x1.ld, x1.col0, y0.form ? 1 : 0);
    }
    case R_ASP_FUSED: {
      // (split16 mode: the same f32 tensors, the logits product on the f16 matrix cores with split operands)
      // (the weights' 2^s: asp_conv.split_scale_inv = 2^-s from the host, data dependent like every other split weight's)
      const float ws = w->asp_conv.split_scale_inv > 0.f ? 1.f / w->asp_conv.split_scale_inv : 256.f;
      return sd_asp_attend_pool_scaled(p[A1], w->asp_conv.w, p[H], x.split ? SD_DT_SPLIT16 : x.dt, Cm, B, T, Cm, w->att_channels, w->asp_eps, ws,
                                       static_cast<float*>(p[POOLED]), x.stream, x.sg.rel_len);
    }
    case R_ASP_POOL: return sd_asp_pool(p[E], Cm, p[H], x.dt, Cm, x.sg, Cm, w->asp_eps, static_cast<float*>(p[POOLED]), x.stream);
    default: break;        // a conv
  }
  const bool per_seg = s.route == R_SEG_GEMM || s.op == OP_SE2;      // B rows of one frame
  const int act = s.op == OP_SE2 ? SD_ACT_SIGMOID : (s.op == OP_ASP_G || s.op == OP_ASP_CONV || s.op == OP_FC) ? SD_ACT_NONE : SD_ACT_RELU;
  sd_conv_args a = conv_of(l, p[x0.buf], dtype_of(x0.form), x0.ld, x0.col0, p[y0.buf], dtype_of(y0.form), y0.ld, y0.col0, per_seg ? B : x.M,
                           per_seg ? 1 : x.Tc, act);
  if (s.wr[1].form) { a.tee = p[s.wr[1].buf]; a.ldt = s.wr[1].ld; a.tee_lo = s.op == OP_TDNN1 ? chunk : 0; a.tee_hi = a.tee_lo + chunk; }
  if (x1.form) { a.tee_add = p[x1.buf]; a.ld_ta = x1.ld; a.ta_col0 = x1.col0; }
  if (s.rd[2].form) { a.bias = static_cast<float*>(p[s.rd[2].buf]); a.bias_per_seg = 1; a.act2 = SD_ACT_TANH; }
  if (s.op == OP_ASP_G) { a.scale = nullptr; a.shift = nullptr; }
  if (s.wr[2].form) { a.colstat = static_cast<float*>(p[s.wr[2].buf]); *stat_rows = 128; }
  switch (s.route) {
    case R_PACKED: return sd_conv1d_cl_packed_f32_with(&a, x.sg.span, B, x.stream, x.tune);
    case R_SEG_GEMM: return sd_seg_gemm_f32_with(&a, p[SKP], x.b.skp_bytes, x.stream, x.tune);
    case R_F32: return sd_conv1d_cl_f32_with(&a, x.stream, x.tune, a.colstat ? stat_rows : nullptr);
    case R_F16: return sd_conv1d_cl_f16_with(&a, x.stream, x.tune);
    case R_SPLIT128: a.w_scale_inv = l.split_scale_inv; break;                 // the layer's own bias / scale
    default: a.bias = l.bias_split; a.scale = l.scale_split; break;            // the folded 2^s vectors
  }
  a.w = l.w_split; a.w_dtype = SD_DT_SPLIT16; a.cin_pad = (l.cin + 31) / 32 * 32;
  return sd_conv1d_cl_split16_with(&a, x.stream, x.tune);
}

#define SD_TRY(expr)            \
  do {                          \
    int e_ = (expr);            \
    if (e_ != SD_OK) return e_; \
  } while (0)

// sg: the segment map of the B segments (SdSegs, sd_common.h).  Check, plan, carve, walk the plan.
int forward(const sd_ecapa_weights* w, const float* feats, const SdSegs& sg, float* emb, void* ws_dev, size_t ws_bytes, sd_stream_t stream, int dt) {
  const int B = sg.B, T = sg.T;
  SD_TRY(check_weights(w, dt));
  SD_CHECK_ARG(B >= 0 && (sg.packed || T > 0), "sd_ecapa_forward: B=%d T=%d", B, T);
  if (B == 0) return SD_OK;
  SD_CHECK_ARG(feats && emb && ws_dev, "sd_ecapa_forward: null feats/emb/workspace");
  SD_CHECK_ARG(sg.packed || (long)B * T < (1L << 31), "sd_ecapa_forward: B*T overflows int");
  SD_CHECK_ARG(sd_aligned16(ws_dev), "sd_ecapa_forward: workspace must be 16-byte aligned");
  const int M = sg.packed ? sg.M : B * T;
  const PlanIn in = {w, B, T, M, sg.packed ? MAP_PACKED : sg.rel_len ? MAP_LENGTHS : MAP_UNIFORM, dt, sd_conv_tuning_now(), switches(), sd_aligned16(feats)};
  Plan plan;
  SD_TRY(make_plan(in, &plan));
  Buffers b = carve(w, B, (size_t)M, ws_dev, dt);
  if (ws_bytes < b.bytes) return sd_set_error(SD_ERR_WORKSPACE, "sd_ecapa_forward: workspace %zu < %zu bytes", ws_bytes, b.bytes);
  b.p[FEATS] = const_cast<float*>(feats);
  b.p[EMB] = emb;
  const Exec x = {w, sg, b, stream, M, in.Tc(), dt, in.split(), in.tune};
  int stat_rows = 128;
  for (int i = 0; i < plan.n; ++i) SD_TRY(run_step(x, plan.s[i], &stat_rows));
  return SD_OK;
}

}  // namespace

extern "C" size_t sd_ecapa_workspace_bytes(const sd_ecapa_weights* w, int B, int T) {
  if (!w || B <= 0 || T <= 0 || w->res2_scale <= 0) return 0;
  return carve(w, B, (size_t)B * T, nullptr, w->w_dtype).bytes;
}

extern "C" size_t sd_ecapa_packed_workspace_bytes(const sd_ecapa_weights* w, int B, int M) {
  if (!w || B <= 0 || M <= 0 || w->res2_scale <= 0) return 0;
  return carve(w, B, (size_t)M, nullptr, SD_DT_F32).bytes;
}

// The plan of one forward as text (sd_hip_trace.h): the rules above, no device
extern "C" size_t sd_ecapa_plan_read(const sd_ecapa_weights* w, int B, int T, int M, int map_kind, char* buf, size_t cap) {
  if (check_weights(w, w ? w->w_dtype : 0) != SD_OK) return 0;
  const bool packed = map_kind == MAP_PACKED;
  if (packed && check_packed_weights(w) != SD_OK) return 0;
  if (map_kind < MAP_UNIFORM || map_kind > MAP_PACKED || B <= 0 || (packed ? M <= 0 : T <= 0 || (long)B * T >= (1L << 31))) {
    sd_set_error(SD_ERR_ARG, "sd_ecapa_plan_read: B=%d T=%d M=%d map_kind=%d", B, T, M, map_kind);
    return 0;
  }
  const PlanIn in = {w, B, packed ? 0 : T, packed ? M : B * T, map_kind, w->w_dtype, sd_conv_tuning_now(0), switches(), true};
  Plan plan;
  if (make_plan(in, &plan) != SD_OK) return 0;
  auto put = [](std::string& t, const TRef* r) {
    for (int k = 0, any = 0; k < 3; ++k)
      if (r[k].form) {
        t += (any++ ? " " : "") + std::string(kBuf[r[k].buf]) + "[" + std::to_string(r[k].col0) + ":" + std::to_string(r[k].col0 + r[k].cols) + "]:" + kForm[r[k].form];
      }
  };
  std::string text = "carve\t-\t\t";
  for (int k = X0; k < EMB; ++k)
    if (k != SKP && has_buf(w, in.dt, k)) text += std::string(k == X0 ? "" : " ") + kBuf[k];
  text += "\n";
  for (int i = 0; i < plan.n; ++i) {
    const Step& s = plan.s[i];
    if (s.blk >= 0) text += "b" + std::to_string(s.blk) + ".";
    if (s.op == OP_PACK) text += std::string(kOp[(int)s.j]) + ".";
    text += kOp[s.op];
    if (s.op == OP_RES2) text += "." + std::to_string(s.j);
    text += std::string("\t") + kRoute[s.route] + "\t";
    put(text, s.rd);
    text += "\t";
    put(text, s.wr);
    text += "\n";
  }
  if (buf && cap) {
    const size_t nb = text.size() < cap - 1 ? text.size() : cap - 1;
    memcpy(buf, text.data(), nb);
    buf[nb] = 0;
  }
  return text.size() + 1;
}

extern "C" int sd_ecapa_forward_packed_f32(const sd_ecapa_weights* w, const float* feats, const int* frame_start_dev, int B, int M, float* emb,
                                           void* ws_dev, size_t ws_bytes, sd_stream_t stream) {
  SD_CHECK_ARG(w != nullptr, "sd_ecapa_forward_packed_f32: null weights");
  SD_TRY(check_packed_weights(w));
  SD_CHECK_ARG(B >= 0, "sd_ecapa_forward_packed_f32: B=%d", B);
  if (B == 0) return SD_OK;
  SD_CHECK_ARG(M > 0 && frame_start_dev != nullptr, "sd_ecapa_forward_packed_f32: M=%d, frame_start %p", M, (const void*)frame_start_dev);
  return forward(w, feats, sd_packed_segs(frame_start_dev, B, M), emb, ws_dev, ws_bytes, stream, SD_DT_F32);
}

extern "C" int sd_ecapa_forward_f32(const sd_ecapa_weights* w, const float* feats, int B, int T, float* emb,
                                    void* ws_dev, size_t ws_bytes, sd_stream_t stream) {
  return forward(w, feats, sd_uniform_segs(B, T), emb, ws_dev, ws_bytes, stream, SD_DT_F32);
}

extern "C" int sd_ecapa_forward_f16(const sd_ecapa_weights* w, const float* feats, int B, int T, float* emb,
                                    void* ws_dev, size_t ws_bytes, sd_stream_t stream) {
  return forward(w, feats, sd_uniform_segs(B, T), emb, ws_dev, ws_bytes, stream, SD_DT_F16);
}

extern "C" int sd_ecapa_forward_lens_f32(const sd_ecapa_weights* w, const float* feats, int B, int T, const float* rel_len_dev, float* emb,
                                         void* ws_dev, size_t ws_bytes, sd_stream_t stream) {
  return forward(w, feats, sd_uniform_segs(B, T, rel_len_dev), emb, ws_dev, ws_bytes, stream, SD_DT_F32);
}

extern "C" int sd_ecapa_forward_lens_f16(const sd_ecapa_weights* w, const float* feats, int B, int T, const float* rel_len_dev, float* emb,
                                         void* ws_dev, size_t ws_bytes, sd_stream_t stream) {
  return forward(w, feats, sd_uniform_segs(B, T, rel_len_dev), emb, ws_dev, ws_bytes, stream, SD_DT_F16);
}
