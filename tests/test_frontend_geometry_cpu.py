"""What tests/test_gpu_frontend_geometry.py stands on, checked without a GPU: the float64 reference of
tests/frontend_cases.py is well conditioned at every clip the GPU test compares, the host tables are the reference's at
every geometry, the case table reaches every code path paths() names, and dr_create refuses a bad geometry before it
asks for a device."""
import ctypes as C

import pytest
import torch

import frontend_cases as FC
from oracle import diffroll_ref as R

# the fp32 reference against the float64 one: observed <= 1.2e-5 at every compared clip of the table
REF_ATOL = 2e-5


@pytest.fixture(scope="module")
def lib():
    from diffroll_amd.build import build
    from diffroll_amd import _cabi
    build(verbose=False)
    return _cabi.load_library()


@pytest.mark.parametrize("c", FC.CASES, ids=FC.case_id)
def test_reference_is_well_conditioned_at_every_compared_clip(c):
    """max |R.frontend (fp32) - frontend64| <= 2e-5 per case, clip and normalisation mode: a comparison of the engine with
    frontend64 at ATOL_SPEC = 4e-5 then measures the engine, not the inputs.  (A condition on the inputs: asserted.)"""
    wav = FC.clips(c)
    assert wav.shape == (4 if c == FC.SILENT_CASE else 3, c.L) and wav.dtype == torch.float32
    for mode in FC.MODES:
        hp = FC.case_hp(c, mode)
        got = R.frontend(wav, hp, 10 ** 9).double()
        power, want = FC.frontend64(wav, hp, mode == "framewise")
        assert got.shape == want.shape == (wav.shape[0], c.n_mels, FC.frames(c))
        assert power.shape == (wav.shape[0], FC.frames(c), c.n_fft // 2 + 1)
        rows = FC.compared_clips(c, mode)
        assert set(range(wav.shape[0])) - set(rows) == ({FC.IMPULSE} if mode == "framewise" else set())
        for b in rows:
            d = float((got[b] - want[b]).abs().max())
            print(f"{FC.case_id(c)} {mode} clip {b}: {d:.3e}")
            assert d <= REF_ATOL, (FC.case_id(c), mode, b, d)
        if c == FC.SILENT_CASE:
            assert bool((want[FC.SILENCE] == 0).all()) and bool((got[FC.SILENCE] == 0).all())


def test_reference_is_well_conditioned_at_the_other_clips_the_gpu_test_runs():
    """The same condition at the clips of the buffer-reuse calls and at the shortest accepted clips."""
    runs = [(FC.REUSE_CASE, B, L, FC.MODES) for B, L in FC.REUSE_CALLS]
    runs += [(c, 3, c.n_fft // 2 + 1, ("imagewise",)) for c in FC.SHORTEST_CASES]
    for c, B, L, modes in runs:
        wav = FC.clips(c, L=L, B=B)
        assert wav.shape == (B, L)
        for mode in modes:
            hp = FC.case_hp(c, mode)
            got = R.frontend(wav, hp, 10 ** 9).double()
            want = FC.frontend64(wav, hp, mode == "framewise")[1]
            rows = FC.compared_clips(c, mode, B)
            d = float((got[rows] - want[rows]).abs().max())
            print(f"{FC.case_id(c)} {mode} B={B} L={L}: {d:.3e}")
            assert d <= REF_ATOL, (FC.case_id(c), mode, B, L, d)


def test_reference_masks_follow_the_oracle():
    """frontend64's masks are the oracle's (model/diffwave.py:649-654): time, frequency, and the rectangle of both."""
    c = FC.CASES[2]
    wav = FC.clips(c)
    hp = FC.case_hp(c)
    for kw in (dict(inpainting_t=[3, 9]), dict(inpainting_f=[6, 40]), dict(inpainting_t=[3, 9], inpainting_f=[6, 40])):
        got = R.frontend(wav, hp, 10 ** 9, **kw)
        want = FC.frontend64(wav, hp, False, **kw)[1]
        assert torch.equal(got == -1, want == -1) and bool((want == -1).any())
        assert float((got.double() - want).abs().max()) <= REF_ATOL


def test_dft_restatement_is_the_same_front_end():
    """dft32_frontend (the fp32 n_fft-term sum a bound for the DFT path may be derived from) computes the front-end: within
    1e-4 of frontend64 at every DFT case - and it is NOT the reference (it differs from it measurably at 2400)."""
    worst = 0.0
    for c in FC.CASES:
        if FC.paths(c)["spectrum"] != "dft":
            continue
        wav = FC.clips(c)
        for mode in FC.MODES:
            hp = FC.case_hp(c, mode)
            got = FC.dft32_frontend(wav, hp, mode == "framewise").double()
            want = FC.frontend64(wav, hp, mode == "framewise")[1]
            rows = FC.compared_clips(c, mode)
            d = float((got[rows] - want[rows]).abs().max())
            print(f"{FC.case_id(c)} {mode}: {d:.3e}")
            assert d <= 1e-4, (FC.case_id(c), mode, d)
            worst = max(worst, d)
    assert worst > 1e-7


@pytest.mark.parametrize("c", FC.CASES, ids=FC.case_id)
def test_frontend_tables_are_the_references_at_every_geometry(c):
    from diffroll_amd.frontend_tables import frontend_tables
    w, norm, fb = frontend_tables(c.n_fft, c.f_min, c.f_max, c.n_mels, c.sample_rate)
    assert w.dtype == fb.dtype == torch.float32 and w.is_contiguous() and fb.is_contiguous()
    assert torch.equal(w, torch.hann_window(c.n_fft)) and norm == float(w.pow(2.0).sum().sqrt())
    assert fb.shape == (c.n_fft // 2 + 1, c.n_mels)
    assert torch.equal(fb, R.melscale_fbanks_htk(c.n_fft // 2 + 1, float(c.f_min), float(c.f_max), c.n_mels, c.sample_rate))


def test_case_table_reaches_every_path():
    seen = {}
    for c in FC.CASES:
        assert c.n_fft % 32 == 0 and c.hop % 4 == 0 and c.n_mels > 0 and c.L > c.n_fft // 2      # accepted by the engine
        assert c.n_fft <= 16384 or c.n_fft & (c.n_fft - 1), "power-of-two n_fft above 16384: a multi-GB DFT matrix"
        for key, val in FC.paths(c).items():
            seen.setdefault(key, set()).add(val)
    for key, want in FC.REQUIRED.items():
        assert want <= seen[key], (key, want - seen[key])
    assert len(seen["bins_p"]) >= 6 and 64 in seen["bins_p"] and 1088 in seen["bins_p"]
    assert len(set(FC.CASES)) == len(FC.CASES) and FC.SILENT_CASE in FC.CASES
    # the paths the issue names, at the rows it names them for
    by = {FC.case_id(c): FC.paths(c) for c in FC.CASES}
    for cid in ("64-16-20-L700", "256-64-40-L4099", "1024-256-80-L16384", "4096-1024-229-L40000", "16384-4096-229-L20481"):
        assert by[cid]["radix2"] is True, cid
    assert by["512-128-64-L8192"]["radix2"] is False and by["2048-500-229-L10000"]["radix2"] is False
    for cid in ("96-24-16-L1000", "1536-384-128-L9001", "2400-600-229-L12000"):
        assert by[cid]["spectrum"] == "dft", cid
    assert by["4096-1024-229-L40000"]["minmax"] == "many" and by["1024-256-83-L25603"]["minmax"] == "many"
    assert by["256-512-130-L6000"]["cond_guard"] and by["256-512-130-L6000"]["hop"] == "beyond"
    # the released geometry, for orientation: everything this table adds is something it does not reach
    rel = FC.paths(FC.Case(2048, 512, 229, 16000, 0, 8000, 64000))
    assert (rel["spectrum"], rel["radix2"], rel["reflect"], rel["mel_tiles"], rel["mel_mod4"], rel["bins_p"]) == ("fft", False, "quad", 2, 1, 1088)


def _config(**kw):
    from diffroll_amd import _cabi
    base = dict(abi_version=_cabi.DR_ABI_VERSION, device=0, residual_channels=64, residual_layers=2, kernel_size=3,
                dilation_base=2, dilation_bound=4, n_mels=229, timesteps=4, sample_rate=16000, n_fft=2048, hop_length=512,
                f_min=0.0, f_max=8000.0, beta_start=1e-4, beta_end=0.02)
    base.update(kw)
    return _cabi.DrConfig(**base)


@pytest.mark.parametrize("kw,text", [(dict(n_fft=48), b"unsupported configuration"), (dict(hop_length=6), b"unsupported configuration"),
                                     (dict(n_mels=0), b"unsupported configuration"), (dict(n_fft=131072), b"configuration too large")],
                         ids=["n_fft48", "hop6", "n_mels0", "n_fft131072"])
def test_bad_geometry_is_refused_before_the_device_is_asked(lib, kw, text):
    from diffroll_amd import _cabi
    cfg = _config(**kw)
    h = C.c_void_p()
    assert lib.dr_create(C.byref(h), C.byref(cfg)) == _cabi.DR_EINVAL and not h.value
    assert text in lib.dr_last_error(None)
