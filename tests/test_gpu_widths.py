"""GPU parity at the widths of Whisper small and medium: d = 768 with 12 heads and d = 1024 with 16 heads.

wmx.engine.MODEL_DIMS offers `small` and `medium`; the other GPU modules run at d = 128, 384, 512 and 1280 only.  What
depends on the width and is reached at these two alone (tests/test_packed_extent.py pins the decode GEMM's share of it
on the CPU, test_small_and_medium_own_plans_in_every_split_mode):
  * the NW = 8 instantiations of gemm_packed_kernel that an unsplit K = d launch takes (K / 32 = 24 or 32 k-steps),
    medium's fc2 on the K >= 4096 -> NCT 4 boundary, the split counts 5, 6 and 7, and all of these again on the 8-bit
    plans, which the CPU walk does not reach;
  * layernorm_mx8_exact_kernel<4, R> (float8, d = 1024) and three full passes of the generic layernorm_mx8_kernel (768);
  * the encoder LayerNorm fold with lng = 3 / 4 statistic groups, 3 / 4 column tiles of the 256-tile GEMM;
  * the fused cross-attention query projection with 3 / 4 k-steps per load batch, head grids of 12 / 16;
  * the row-major GEMM dispatch below and exactly on the N >= 1024 skinny threshold;
  * reduce_ln4_kernel with 3 / 4 waves.
Models: one encoder layer and two decoder layers (layer 0's last reduce + LayerNorm chains into layer 1 in the mixed
step), PRNG weights of seed 5; audio synth.speech_like(100 + i, n) with n = 480000, 150000, 320000, 16000.  Every
model and context is created with WMX_GUARD=1 (a 64 KiB patterned gap after every arena buffer) and every test ends
with wmx_debug_guard_check == (-1, -1): no launch wrote past its buffer.

Bounds are the project's (tests/test_gpu_parity.py, test_gpu_step.py, test_gpu_mx8.py, test_gpu_int8.py): relative L2
bf16 <= 3e-2, f16 <= 5e-3, MX-fp8 encoder <= 3e-2; argmax equal wherever the oracle's top-2 margin exceeds twice the
row's max abs error, with >= 16 of 25 steps compared per row in f16.  The floor is met by the reference alone: the
oracle's margin exceeds 0.3 on at least 23 of the 25 steps of every row for each f16 stream below (R = 20 and R = 3 on
the 16-bit weights, R = 20 on the int8 grid; computed on the CPU for both widths), so the floor can fail only if the
device's max abs logit error exceeds 0.15.

Measured on the first green run (MI355X), worst relative L2 per width and dtype (768 | 1024):
  encoder, three windows          bf16 1.93e-3 | 1.92e-3 (3e-2)    f16 2.41e-4 | 2.39e-4 (5e-3)
  encoder, one window             bf16 1.82e-3 | 1.81e-3           f16 2.27e-4 | 2.27e-4
  fold's cost, bf16               folded 1.93e-3 vs unfolded 1.82e-3 | 1.92e-3 vs 1.81e-3 (bound 3 x unfolded + 2e-3)
  decoder logits, T = 5 and 21    bf16 3.47e-3 | 3.38e-3           f16 4.42e-4 | 4.25e-4
  forced steps R = 20             bf16 3.69e-3 | 3.65e-3           f16 4.60e-4 | 4.48e-4
  forced steps R = 3              bf16 3.69e-3 | 3.52e-3           f16 4.60e-4 | 4.36e-4
  R = 40 / R = 20 padded, bf16    3.70e-3 / 3.69e-3 | 3.70e-3 / 3.69e-3
  fast step, separate cross-q     bf16 3.57e-3 | 3.53e-3           f16 4.50e-4 | 4.40e-4 (both variants alike)
  MX-fp8 encoder                  6.04e-3 | 6.17e-3 (3e-2, and q / 2 = 9.3e-3 | 8.7e-3)
  fp8 decode R = 20 / R = 3       3.43e-3 / 3.35e-3 | 3.39e-3 / 3.39e-3 (3e-2); vs 16-bit weights 5.4e-2 | 4.9e-2
  int8 decode R = 20              4.32e-4 | 4.33e-4 (5e-3); vs 16-bit weights 8.1e-3 | 7.4e-3 (> 5e-3)
  alignment matrix, f16           2.31e-3 | 2.22e-3 (5e-3), 31 text tokens, all jump times within one frame
Argmax compared on 25 of 25 steps in every f16 row (bf16 and fp8: at least 23); the 32-step beam-5 search replayed in
full on both windows with no float tie, in bf16 and f16.
"""
import contextlib
import ctypes as C
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import whisper_np as O
from wmx import synth

pytestmark = pytest.mark.gpu

W768 = O.Dims(80, 51865, 768, 12, 1, 768, 12, 2)
W1024 = O.Dims(80, 51865, 1024, 16, 1, 1024, 16, 2)
WIDTHS = {768: W768, 1024: W1024}
LENS = (480000, 150000, 320000, 16000)
SEED = 5
N_STEPS = 24
CT = {"bf16": "bfloat16", "f16": "float16", "float8": "float8", "int8": "int8_float16"}
ODT = {"bf16": "bf16", "f16": "f16", "float8": "bf16", "int8": "f16"}  # the oracle's weight rounding per compute type


# ---------------------------------------------------------------------------------------------------------------
# creation under WMX_GUARD=1 (and the switches a test selects), and the guard check every test ends with
# ---------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _env(**kv):
    """Environment switches the library reads at model / context creation, restored afterwards."""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _model(d, ct, **switches):
    from wmx import engine as E
    import test_gpu_step as S
    with _env(WMX_GUARD="1", **switches):
        m = E.Model(S._edims(d), 0, CT[ct])
    return m.init_synthetic(SEED)


def _context(m, **kw):
    from wmx import engine as E
    switches = kw.pop("switches", {})
    with _env(WMX_GUARD="1", **switches):
        return E.Context(m, **kw)


def _guard_ok(m, *ctxs):
    """No guard gap of the model's arena or of the contexts' buffers was written (wmx_debug_guard_check)."""
    from wmx._lib import check, lib
    for ctx in ctxs:
        mb, cb = C.c_int(), C.c_int()
        check(lib.wmx_debug_guard_check(m._h, ctx._h, C.byref(mb), C.byref(cb)))
        assert (mb.value, cb.value) == (-1, -1), ("guard gap overwritten after (model, context) buffer", mb.value,
                                                  cb.value)


# ---------------------------------------------------------------------------------------------------------------
# references, computed once and shared (never modified)
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _audios():
    return tuple(synth.speech_like(100 + i, n) for i, n in enumerate(LENS))


@functools.lru_cache(maxsize=None)
def _mels():
    return np.stack([O.logmel_segment(a, 80) for a in _audios()])


@functools.lru_cache(maxsize=None)
def _weights(width, odt):
    return O.make_weights(WIDTHS[width], SEED, odt)


@functools.lru_cache(maxsize=None)
def _encs(width, odt, mx8=False):
    return tuple(O.encoder(_weights(width, odt), WIDTHS[width], mel, mx8=mx8) for mel in _mels())


def _stream(shape, n_vocab):
    """(B, K, prefix, tokens, parents) of a teacher-forced stream: r20 = 4 windows x beam 5, r3 = 3 windows greedy,
    r40 = 8 windows x beam 5 (the four windows twice), r20pad = r20 behind left-padded prompts of lengths 0, 5, 11, 2."""
    import test_gpu_step as S
    sp = O.special_tokens(n_vocab)
    B, K, seed = {"r20": (4, 5, 2), "r3": (3, 1, 2), "r40": (8, 5, 6), "r20pad": (4, 5, 2)}[shape]
    tok, par = S._forced_stream(np.random.default_rng(seed), N_STEPS, B * K, K)
    prefix = [[sp.sot, sp.lang0, sp.transcribe]] * B
    if shape == "r20pad":
        prefix = [[sp.sot_prev] + list(range(1000, 1000 + L)) + [sp.sot, sp.lang0, sp.transcribe] for L in (0, 5, 11, 2)]
        prefix[0] = [sp.sot, sp.lang0, sp.transcribe]
    return B, K, prefix, tok, par


@functools.lru_cache(maxsize=None)
def _forced_ref(width, odt, shape):
    """O.forced_rows of a stream on the 16-bit weights and the oracle's own encoder output."""
    d = WIDTHS[width]
    B, K, prefix, tok, par = _stream(shape, d.n_vocab)
    encs = (_encs(width, odt) * 2)[:B]
    return O.forced_rows(_weights(width, odt), d, encs, prefix, tok, par, K)


@functools.lru_cache(maxsize=None)
def _bundle(width, ct):
    """The device model of one (width, compute type) with its oracle weights."""
    d = WIDTHS[width]
    return SimpleNamespace(width=width, d=d, ct=ct, odt=ODT[ct], m=_model(d, ct), W=_weights(width, ODT[ct]),
                           sp=O.special_tokens(d.n_vocab))


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for f in (_bundle, _forced_ref, _encs, _weights):
        f.cache_clear()


PAIRS16 = [(w, dt) for w in WIDTHS for dt in ("bf16", "f16")]


@pytest.fixture(scope="module", params=PAIRS16, ids=lambda p: f"{p[0]}-{p[1]}")
def wm(request):
    return _bundle(*request.param)


@pytest.fixture(scope="module", params=list(WIDTHS), ids=str)
def wm_bf16(request):
    return _bundle(request.param, "bf16")


@pytest.fixture(scope="module", params=list(WIDTHS), ids=str)
def wm_fp8(request):
    return _bundle(request.param, "float8")


@pytest.fixture(scope="module", params=list(WIDTHS), ids=str)
def wm_int8(request):
    return _bundle(request.param, "int8")


# ---------------------------------------------------------------------------------------------------------------
# 1. encoder, 16-bit
# ---------------------------------------------------------------------------------------------------------------
def _encode_both_shapes(b, refs, tag, bound):
    """Three windows in one batch (4500 rows) and single windows (1500 rows) against refs; returns the contexts and
    the three-window output."""
    from test_gpu_parity import rel_l2
    mels = _mels()
    ctx3 = _context(b.m, max_batch=3, beam_size=1, max_new_tokens=8, word_timestamps=False)
    got3 = ctx3.encode(mels[:3])
    errs = [rel_l2(got3[i], refs[i]) for i in range(3)]
    ctx1 = _context(b.m, max_batch=1, beam_size=1, max_new_tokens=8, word_timestamps=False)
    errs1 = {i: rel_l2(ctx1.encode(mels[i:i + 1])[0], refs[i]) for i in (3, 0)}
    print(f"{tag}: encoder rel_l2, three windows {['%.2e' % e for e in errs]}, alone "
          f"{ {i: '%.2e' % e for i, e in errs1.items()} } (bound {bound})")
    for e in errs + list(errs1.values()):
        assert e <= bound, (tag, errs, errs1)
    return (ctx3, ctx1), got3, errs


def test_encoder_matches_oracle(wm):
    """Three windows (256 x 256 tile, LayerNorms folded with lng = 3 / 4, cross-K/V scatter epilogue) and one window
    (128 x 128 tile, LayerNorm launches); bf16 also against the same model with the fold off: the fold's own cost."""
    import test_gpu_step as S
    from test_gpu_parity import rel_l2
    b = wm
    refs = _encs(b.width, b.odt)
    ctxs, got3, errs = _encode_both_shapes(b, refs, f"d {b.width} {b.ct}", S.REL[b.ct])
    _guard_ok(b.m, *ctxs)
    if b.ct == "bf16":
        m0 = _model(b.d, "bf16", WMX_ENC_FOLD="0")
        ctx0 = _context(m0, max_batch=3, beam_size=1, max_new_tokens=8, word_timestamps=False)
        got0 = ctx0.encode(_mels()[:3])
        for i in range(3):
            e0, ef = rel_l2(got0[i], refs[i]), rel_l2(got3[i], got0[i])
            print(f"d {b.width} bf16 window {i}: folded {errs[i]:.3e}, unfolded {e0:.3e}, folded vs unfolded {ef:.3e}")
            assert errs[i] <= 3 * e0 + 2e-3, (i, errs[i], e0)  # the fold may not dominate the error budget
        _guard_ok(m0, ctx0)
        ctx0.close()
        m0.close()


# ---------------------------------------------------------------------------------------------------------------
# 2. decoder forward (prefill path)
# ---------------------------------------------------------------------------------------------------------------
def test_decoder_logits_match_oracle(wm):
    """Three windows at T = 5 (key-chunked cross attention) and T = 21 (> 16 queries): the row-major projections below
    (768) and on (1024) the skinny tile's N >= 1024 threshold."""
    import test_gpu_step as S
    from test_gpu_parity import rel_l2
    b = wm
    encs = _encs(b.width, b.odt)
    ctx = _context(b.m, max_batch=3, beam_size=1, max_new_tokens=8, word_timestamps=False)
    ctx.encode(_mels()[:3], want_output=False)
    rng = np.random.default_rng(11)
    for T in (5, 21):
        toks = np.concatenate([np.full((3, 1), b.sp.sot, np.int32),
                               rng.integers(0, 50000, size=(3, T - 1)).astype(np.int32)], axis=1)
        got = ctx.decoder_logits(toks)
        for i in range(3):
            ref = O.decoder_forward(b.W, b.d, list(toks[i]), O.DecoderCache(b.W, b.d, encs[i]))
            e = rel_l2(got[i], ref)
            print(f"d {b.width} {b.ct} decoder logits T {T} window {i} rel_l2 {e:.2e}")
            assert e <= S.REL[b.ct], (T, i, e)
    _guard_ok(b.m, ctx)


# ---------------------------------------------------------------------------------------------------------------
# 3. decode step, teacher-forced
# ---------------------------------------------------------------------------------------------------------------
def _forced_on_device(b, shape, m=None, switches=None):
    """The stream of `shape` on the device (the oracle's windows encoded by the device) against _forced_ref."""
    import test_gpu_step as S
    m = m or b.m
    B, K, prefix, tok, par = _stream(shape, b.d.n_vocab)
    ctx = _context(m, max_batch=B, beam_size=K, max_new_tokens=64, word_timestamps=False, switches=switches or {})
    ctx.encode(np.concatenate([_mels()] * 2)[:B], want_output=False)
    top1, lg = ctx.forced_decode(prefix, tok, par, logits_every=1)
    ref_top1, ref_margin, ref_lg = _forced_ref(b.width, b.odt, shape)
    tag = f"d {b.width} {shape}" + "".join(f" {k}={v}" for k, v in (switches or {}).items())
    S._check_forced(tag, b.ct, top1, lg, 1, ref_top1, ref_margin, ref_lg, 16)
    _guard_ok(m, ctx)


@pytest.mark.parametrize("shape", ["r20", "r3"])
def test_forced_steps(wm, shape):
    """4 windows x beam 5 (R = 20, MT 2, parents redrawn every step) and 3 windows greedy (R = 3, MT 1), 24 steps on the
    mixed step: the NW = 8 packed plans, the fused cross-q projection, reduce_ln4 with 3 / 4 waves."""
    _forced_on_device(wm, shape)


@pytest.mark.parametrize("shape", ["r40", "r20pad"])
def test_forced_steps_bf16_shapes(wm_bf16, shape):
    """8 windows x beam 5 (R = 40, MT 3, the M > 24 split target) and R = 20 behind left-padded prompts."""
    _forced_on_device(wm_bf16, shape)


def test_forced_steps_fast_step(wm):
    """R = 20 on the fast step (WMX_DEC_MIXED=0 at model creation): every d x d projection split-K + reduce_ln."""
    b = wm
    m0 = _model(b.d, b.ct, WMX_DEC_MIXED="0")
    _forced_on_device(b, "r20", m=m0, switches={"WMX_DEC_MIXED": "0"})
    m0.close()


def test_forced_steps_separate_cross_q(wm):
    """R = 20 with the cross-q projection as its own split-K launch (WMX_XQ_FUSED=0 at context creation)."""
    _forced_on_device(wm, "r20", switches={"WMX_XQ_FUSED": "0"})


# ---------------------------------------------------------------------------------------------------------------
# 4. float8 model
# ---------------------------------------------------------------------------------------------------------------
def test_mx8_encoder_matches_oracle(wm_fp8):
    """The 256-tile MX-fp8 GEMM on three windows and the small tiles on one, behind layernorm_mx8_exact_kernel<4> (1024)
    or the generic kernel's three 256-column passes (768), against the oracle's MX rule on bf16-rounded weights.

    Beside the 3e-2 of test_gpu_mx8.test_mx8_encoder_matches_oracle, the criterion of its full-depth test, stated on the
    reference alone: q = rel-L2 between the oracle's MX-fp8 encoder and its 16-bit encoder is what the MX rule itself
    moves the output by (1.85e-2 at 768, 1.73e-2 at 1024, one layer), and a device that follows the rule sits within
    q / 2 of the MX oracle.  A LayerNorm that is 3 % off (a divisor d + 32 in layernorm_mx8_exact_kernel: less than one
    e4m3 step, so 3e-2 alone does not see it) measured 1.8e-2 at 1024 against 6.2e-3 for the sound kernel."""
    from test_gpu_parity import rel_l2
    b = wm_fp8
    refs = _encs(b.width, "bf16", True)
    ctxs, got3, errs = _encode_both_shapes(b, refs, f"d {b.width} float8", 3e-2)
    for i in range(3):
        q = rel_l2(refs[i], _encs(b.width, "bf16")[i])
        print(f"d {b.width} float8 window {i}: rel_l2 {errs[i]:.2e} against q / 2 = {q / 2:.2e}")
        assert errs[i] <= 0.5 * q, (i, errs[i], q)
    _guard_ok(b.m, *ctxs)


def _quantized_forced(b, Wq, W16, B, K, tag, min_cmp):
    """A teacher-forced stream of a model with 8-bit decoder weights against the oracle on Wq and the DEVICE's encoder
    output (the comparison isolates the decoder); and its distance to the 16-bit weights W16: the grid is live."""
    import test_gpu_step as S
    from test_gpu_parity import rel_l2
    shape = "r20" if K == 5 else "r3"
    _, _, prefix, tok, par = _stream(shape, b.d.n_vocab)
    ctx = _context(b.m, max_batch=B, beam_size=K, max_new_tokens=64, word_timestamps=False)
    encs = list(ctx.encode(_mels()[:B]))
    top1, lg = ctx.forced_decode(prefix, tok, par, logits_every=1)
    ref_top1, ref_margin, ref_lg = O.forced_rows(Wq, b.d, encs, prefix, tok, par, K)
    S._check_forced(f"d {b.width} {tag} {shape}", "f16" if b.ct == "int8" else "bf16", top1, lg, 1, ref_top1, ref_margin,
                    ref_lg, min_cmp)
    _, _, lg16 = O.forced_rows(W16, b.d, encs[:1], prefix[:1], tok[:2, :K], par[:2, :K], K)
    d16 = rel_l2(lg[1, 0], lg16[1][0])
    print(f"d {b.width} {tag} vs the 16-bit weights, row 0 step 1 rel_l2 {d16:.2e}")
    assert d16 > 5e-3, d16
    _guard_ok(b.m, ctx)


@pytest.mark.parametrize("B,K", [(4, 5), (3, 1)])
def test_fp8_decode_forced_steps(wm_fp8, B, K):
    """The fp8 decode (e4m3 weights with a row scale, fp8 cross-K/V images) on its 8-bit packed plans (packed_ku8, the
    80 KiB LDS budget), which the CPU walk does not reach."""
    b = wm_fp8
    _quantized_forced(b, O.fp8_decoder_weights(b.W, b.d), b.W, B, K, "fp8 decode", 16)


def _int8_kept(d):
    import test_gpu_int8 as I8
    return I8._kept(d)


def test_int8_forced_decode_matches_oracle(wm_int8):
    """The CTranslate2 int8 grid derived on the device from the synthetic weights (scales read back), R = 20."""
    b = wm_int8
    scales = {name: b.m.get_int8(name, shape)[1] for name, shape in _int8_kept(b.d).items()}
    _quantized_forced(b, O.int8_decoder_weights(b.W, b.d, scales), b.W, 4, 5, "int8 decode", 16)


# ---------------------------------------------------------------------------------------------------------------
# 6. free-running search and word alignment through hipGraph replay
# ---------------------------------------------------------------------------------------------------------------
ALIGN_WINDOWS = (0, 2)


def test_search_replay_and_alignment(wm):
    """Two windows x beam 5 with word timestamps: the recorded 32-step search replayed token-exact by the oracle; in
    f16 the alignment matrix of the first window (cross_scores_kernel over the 12 / 16 heads of decoder layer 1) by
    the criteria of test_gpu_parity.test_word_alignment_matrix_micro."""
    import test_gpu_step as S
    from test_gpu_align import _jumps, _lib_dtw
    from test_gpu_parity import rel_l2
    b = wm
    sp = b.sp
    audios = [_audios()[i] for i in ALIGN_WINDOWS]
    ctx = _context(b.m, max_batch=2, beam_size=5, max_new_tokens=32, word_timestamps=True, language=sp.lang0)
    ctx.record(33)
    res = ctx.transcribe(audios)
    opt = O.DecodeOptions(language=sp.lang0, beam_size=5, max_new_tokens=32)
    S._replay_and_compare(f"d {b.width} {b.ct} beam5 B=2", ctx, res, 5, opt, sp, 16)
    assert all(r.jump_times is not None for r in res)
    if b.ct == "f16":
        r = res[0]
        text = [t for t in r.tokens if t < sp.eot]
        assert len(text) >= 16, r.tokens
        enc = _encs(b.width, b.odt)[ALIGN_WINDOWS[0]]
        ti, tj, probs, jt, ref = O.find_alignment(b.W, b.d, enc, sp.lang0, "transcribe", text, r.seek_frames,
                                                   return_matrix=True)
        dev = ctx.alignment_matrix(0)
        assert dev.shape == ref.shape, (dev.shape, ref.shape)
        e = rel_l2(dev, ref)
        np.testing.assert_array_equal(r.jump_times, _jumps(*_lib_dtw(dev)).astype(np.float32))
        assert len(r.jump_times) == len(jt) == len(text) + 1
        within = float(np.mean(np.abs(r.jump_times - jt) <= 0.02 + 1e-6))
        print(f"d {b.width} f16 alignment: {len(text)} text tokens, matrix rel_l2 {e:.2e}, jump times within 1 frame "
              f"{within:.3f}")
        assert e <= S.REL["f16"], e
        assert within >= 0.95, (r.jump_times, jt)
    _guard_ok(b.m, ctx)
