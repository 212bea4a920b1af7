"""Inputs and references along the MAGNITUDE axis, shared by tests/test_gpu_scale.py, tests/test_scale_rules.py and
tools/split16_scale.py (which writes profiles/split16_scale.json):

  * random (inexact) conv cases on the shapes of exact_cases.py, for the metamorphic identity "the output at 2^e is ldexp of the output
    at 2^0": every operation of the operators is homogeneous of degree one in x, bias, shift and tee_add, and a power of two commutes
    with every rounding while nothing leaves the normal range;
  * the accuracy cases of the split operators with EVERY channel of x at 2^e, their float64 reference and the numpy emulation of the
    header's arithmetic (exact_cases.split16_conv_sum);
  * the quiet / loud twin of a state dict: all frame-level activations c times their size, the embedding unchanged."""
import numpy as np

import exact_cases as E

ACCURACY_EXPONENTS = (0, -4, -8, -12)
# (B, T, cin, cout, k, dil): the wide form (x packed by sd_split16_pack_f32, the 256x256 kernel) and the narrow one (split while staged)
ACCURACY_SHAPES = {"wide": (2, 131, 96, 1024, 1, 1), "narrow": (3, 57, 128, 128, 3, 2)}
ENGINE_SCALES = (2.0 ** -8, 2.0 ** 5)
ENGINE_PRECISIONS = ("f32", "f32ns", "f32s", "f16")


def f32(a):
    """Rounded to f32, held as float64 (what the device receives, and what the references must start from)."""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def random_conv(name, f16=False, seed=0):
    """A random case on the shape and the epilogue of exact case `name` (per-segment bias, tee and tee_add as there; relu).  f32: normal
    x, w / sqrt(fan in), bias, scale in [0.5, 1.5), shift.  `f16`: every stored value an exact f16 of magnitude in [2^-2, 2^3) -- x,
    tee_add, and, as the shift is in [1, 2) behind a relu and a positive scale, y and tee >= 1: no value of the run at 2^-4 is an f16
    subnormal, where the grid is absolute and the identity does not hold.  The expected outputs stay empty: the identity needs none."""
    s = E.SHAPES[name.split("-")[0]]
    per_seg, _, tee, add = E.DENSE[name]
    rng = np.random.default_rng(seed + 7 * s["cout"] + s["cin"])
    lengths = E._lengths(s)
    M, B, cin, cout, k = sum(lengths), len(lengths), s["cin"], s["cout"], s["k"]

    def values(shape):
        if not f16:
            return f32(rng.standard_normal(shape))
        return rng.choice(np.array([-1.0, 1.0]), shape) * rng.integers(1024, 2048, shape) * 2.0 ** rng.integers(-12, -7, shape)

    w = rng.standard_normal((cout, cin, k)) / np.sqrt(cin * k) / (8.0 if f16 else 1.0)
    c = E.ConvCase(name + "-random", "dense", lengths, "spans" in s, cin, cout, k, s["dil"], values((M, cin)),
                   (w.astype(np.float16) if f16 else w.astype(np.float32)).astype(np.float64),
                   bias=f32(rng.standard_normal((B, cout) if per_seg else (cout,))), bias_per_seg=per_seg, act="relu",
                   scale=f32(rng.uniform(0.5, 1.5, cout)), shift=f32(rng.uniform(1.0, 2.0, cout) if f16 else rng.standard_normal(cout)))
    if tee:
        c.tee_lo, c.tee_hi = tee
        if add:
            c.tee_add = np.abs(values((M, tee[1] - tee[0]))) if f16 else values((M, tee[1] - tee[0]))
    if f16:
        E.need_f16(c.name, c.x, c.w, *([c.tee_add] if c.tee_add is not None else []))
    return c


def at_scale(c, e):
    """Case `c` with x, bias, shift and tee_add times 2^e (exact)."""
    t = E.ConvCase(**c.__dict__)
    t.x, t.bias, t.shift, t.tee_add = E.scaled(e, c.x, c.bias, c.shift, c.tee_add)
    return t


def random_chain(B, T, dil, n=7, ld=1024 + 64, seed=0):
    """(r, layers) for the Res2Net chain with f16-exact operands: r in [2^-2, 2^3), weights of about 1 / 32, shift in [1, 2) behind a
    relu, so that every chain state is at least 1 and below 2^7 (no f16 subnormal at 2^-4, no overflow at 2^4)."""
    rng = np.random.default_rng(seed + T + dil)
    r = rng.integers(1024, 2048, (B * T, ld)) * 2.0 ** rng.integers(-12, -7, (B * T, ld))
    layers = [dict(w=(rng.standard_normal((128, 128, 3)) / 32.0 / np.sqrt(384.0)).astype(np.float16).astype(np.float64),
                   bias=f32(rng.standard_normal(128) * 0.1), scale=f32(rng.uniform(0.5, 1.0, 128)), shift=f32(rng.uniform(1.0, 2.0, 128)), dil=dil)
              for _ in range(n)]
    return r, layers


# ------------------------------------------------------------------ accuracy of the split operators as a function of scale

def accuracy_case(form, e, seed=0):
    """-> (x [M, cin] at 2^e, w [cout, cin, k], T, dil, the float64 conv, the emulated split conv): Gaussian x with EVERY channel times
    2^e, w normal / sqrt(fan in) as in tests/test_gpu_split16.py; no bias and no activation, so that the largest output moves with
    the scale and the bar stays relative to it."""
    B, T, cin, cout, k, dil = ACCURACY_SHAPES[form]
    rng = np.random.default_rng(seed + cout + cin)
    x = np.ldexp(f32(rng.standard_normal((B * T, cin)) * 3.0), e)
    w = f32(rng.standard_normal((cout, cin, k)) / np.sqrt(cin * k))
    src = E.source_rows((T,) * B, k, dil)
    return x, w, T, dil, E.conv_sum(x, w, src), E.split16_conv_sum(x, w, src)


def accuracy_bar(ref, emulated):
    """(the emulation's error, the bar): the kernel may miss float64 by twice what the header's own arithmetic misses it by (the factor
    2 is for the order of the f32 sums) plus 2e-6 of the largest output, the exact-f32 operator's bar."""
    e_emul = float(np.abs(emulated - ref).max())
    return e_emul, 2.0 * e_emul + 2e-6 * float(np.abs(ref).max())


def measure_accuracy(dev, form, e):
    """One launch of the split operator on `accuracy_case(form, e)` -> dict(scale, top, measured, emulated, bar)."""
    import torch
    from speech_diarization_amd import ops
    x, w, T, dil, ref, emul = accuracy_case(form, e)
    ws, s = ops.pack_weight_split16(w, dev)
    got = ops.conv1d_cl_split16(torch.from_numpy(x).float().to(dev), ws, s, T, cin=x.shape[1], dil=dil, narrow=form == "narrow")
    torch.cuda.synchronize()
    e_emul, bar = accuracy_bar(ref, emul)
    return dict(form=form, log2_scale=e, top=float(np.abs(ref).max()), measured=float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max()),
                emulated=e_emul, bar=bar)


# ------------------------------------------------------------------ the quiet / loud twin of a state dict

def scaled_state_dict(sd, c):
    """All frame-level activations c times their size, the embedding the same function of the input (up to BN_EPS, which is not scaled):
    for every frame-level conv + BN (stem, tdnn1, the Res2Net convs, tdnn2, MFA) the conv bias, the BN weight, bias and running mean
    times c and the running variance times c^2; the stem's conv weight times c; and, where a per-segment layer reads frame-level
    values, the inverse: se_block.conv1 and the attention TDNN's conv weight / c, asp_bn's running mean times c and variance times
    c^2.  c a power of two: every product is exact in f32."""
    out = {k: np.array(v, copy=True) for k, v in sd.items()}
    mul = lambda k, f: out.__setitem__(k, (out[k].astype(np.float64) * f).astype(out[k].dtype))  # noqa: E731
    for key in sd:
        if not key.endswith(".norm.running_var") or key.startswith(("asp.tdnn.", "asp_bn.")):
            continue
        bn = key[:-len(".running_var")]                     # "....norm.norm"
        conv = bn[:-len(".norm.norm")] + ".conv.conv"
        for k in (conv + ".bias", bn + ".weight", bn + ".bias", bn + ".running_mean"):
            mul(k, c)
        mul(key, c * c)
    mul("blocks.0.conv.conv.weight", c)
    for key in sd:
        if key.endswith(".se_block.conv1.conv.weight") or key == "asp.tdnn.conv.conv.weight":
            mul(key, 1.0 / c)
    mul("asp_bn.norm.running_mean", c)
    mul("asp_bn.norm.running_var", c * c)
    return out


def cos_dist(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return 1.0 - (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
