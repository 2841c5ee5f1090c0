"""Host tests of the windowed whole-clip call (include/ext/fsnp_windowed.h): the plan's properties by brute force, the float restatement
of the merge, fsnp_window_count, the second ctypes registry (fullsubnet_plus_amd/_lib_ext.py) against its header, the header as plain
C, and the Python refusals that need no GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import fullsubnet_plus_amd
from fullsubnet_plus_amd import FullSubNet, FullSubNet_Plus, _build, _lib, _lib_ext
from fullsubnet_plus_amd.synthetic import DEFAULT_MODEL_ARGS, FULLSUBNET_MODEL_ARGS
from tests._windowed_util import fade, merge, window_plan
from tests.test_host_abi_signatures import mismatches, parse_prototypes, table_classes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF = 256                                   # n_fft / 2 of the default geometry: the smallest overlap
WINDOWS = (1024, 1500, 2048, 4096)


def _overlaps(W):
    return sorted(set(range(HALF, W // 2 + 1, 37)) | {W // 2})


def _lengths(W, V):
    """Every L in (n_fft / 2, 3 W] for the two small windows; for the large ones every L within 2 of a window's start, of the end of
    an overlap and of a window's end, and every 97th in between."""
    if W <= 1500:
        return range(HALF + 1, 3 * W + 1)
    S = W - V
    edges = {HALF + 1, 3 * W}
    for k in range(3 * W // S + 2):
        for e in (k * S, k * S + V, k * S + W):
            edges.update(range(e - 2, e + 3))
    edges.update(range(HALF + 1, 3 * W + 1, 97))
    return sorted(L for L in edges if HALF < L <= 3 * W)


@pytest.mark.parametrize("W", WINDOWS)
def test_plan_properties_by_brute_force(W):
    plans = 0
    for V in _overlaps(W):
        S = W - V
        for L in _lengths(W, V):
            plan = window_plan(L, W, V)
            K = len(plan)
            cover = np.zeros(L + 1, dtype=np.int64)
            for a, n in plan:
                cover[a] += 1
                cover[a + n] -= 1
            cover = np.cumsum(cover[:L])
            assert cover.min() >= 1 and cover.max() <= 2, (W, V, L)                        # every sample in one or two windows
            assert all(n == W for _, n in plan[:-1]), (W, V, L)                            # every window but the last is full
            assert plan[-1][0] + plan[-1][1] == L and 0 < plan[-1][1] <= W, (W, V, L)      # the last one ends at L
            if K > 1:
                assert plan[-1][1] > V >= HALF, (W, V, L)                                  # ... and is a clip of its own
                two = np.flatnonzero(cover == 2)
                want = np.concatenate([np.arange(k * S, min(k * S + V, L)) for k in range(1, K)])
                assert np.array_equal(two, want), (W, V, L)                                # windows k - 1, k share exactly [k S, k S + V)
            plans += 1
    assert plans > 1000


def test_merge_of_the_clips_own_windows_is_the_clip():
    rng = np.random.default_rng(5)
    for W, V, L in ((4096, 1024, 10000), (4096, 2048, 10000), (1500, 293, 4499), (1024, 256, 1281), (1024, 512, 700)):
        x = (rng.standard_normal(L) * 10.0 ** rng.integers(-3, 3, size=L)).astype(np.float32)
        rows = [x[a:a + n] for a, n in window_plan(L, W, V)]
        got = merge(rows, L, W, V, np.float32)
        assert got.dtype == np.float32 and np.array_equal(got, x), (W, V, L)


def test_merge_fades_between_two_constant_windows():
    W, V, L = 1024, 256, 1500
    rows = [np.full(1024, 1.0), np.full(L - 768, 3.0)]
    got = merge(rows, L, W, V)
    assert np.all(got[:768] == 1.0) and np.all(got[1024:] == 3.0)
    assert np.allclose(got[768:1024], 1.0 + 2.0 * fade(V), rtol=0, atol=1e-15) and got[768] == 1.0


@pytest.mark.parametrize("V", [256, 293, 1024, 2048, 8192])
def test_fade_is_complementary(V):
    g = fade(V)
    assert g[0] == 0.0 and np.all(np.diff(g) > 0)
    j = np.arange(1, V)
    assert np.abs(g[j] + g[V - j] - 1.0).max() < 1e-15
    if V % 2 == 0:
        # at V = W / 2 this is the second half-period of the periodic Hann window of 2 V points: the reference's overlapped_chunk
        assert np.abs(g - torch.hann_window(2 * V, periodic=True, dtype=torch.float64).numpy()[:V]).max() < 1e-15


def test_window_count_matches_the_plan_without_a_gpu():
    lib = _lib.load()
    checked = 0
    for W in WINDOWS:
        for V in _overlaps(W):
            for L in _lengths(W, V):
                K = len(window_plan(L, W, V))
                assert lib.fsnp_window_count(L, W, V) == K == fullsubnet_plus_amd.window_count(L, W, V), (L, W, V)
                checked += 1
    assert checked > 1000
    assert lib.fsnp_window_count(5_000_000, 65536, 8192) == 88 and lib.fsnp_window_count(2 ** 40, 4096, 1024) == -(-(2 ** 40 - 1024) // 3072)
    for bad in ((10000, 1, 1), (10000, 4096, 0), (10000, 4096, 2049), (10000, 4096, -5), (0, 4096, 1024), (-3, 4096, 1024), (10000, -8, 1)):
        assert lib.fsnp_window_count(*bad) == -1, bad
        with pytest.raises(ValueError, match="window_count"):
            fullsubnet_plus_amd.window_count(*bad)
    assert lib.fsnp_window_count(10000, 2, 1) == 9999 and fullsubnet_plus_amd.window_count(1, 2, 1) == 1


# ------------------------------------------------------------------------------------------------ the second registry
def test_extension_header_matches_its_table_type_by_type():
    assert set(_lib_ext.EXT_HEADER_TABLES) == {"ext/fsnp_windowed.h"}
    on_disk = {"ext/" + f for f in os.listdir(os.path.join(ROOT, "include", "ext")) if f.endswith(".h")}
    assert on_disk == set(_lib_ext.EXT_HEADER_TABLES)
    for header, table in _lib_ext.EXT_HEADER_TABLES.items():
        with open(os.path.join(ROOT, "include", header)) as f:
            declared = parse_prototypes(f.read())
        assert len(declared) == len(table) == 3
        assert mismatches(declared, table_classes(table)) == [], header
    assert set(_lib_ext.WINDOWED_SYMBOLS) == {"fsnp_window_count", "fsnp_enhance_wave_windowed", "fsnp_debug_window_roundtrip"}


def test_the_two_registries_share_no_name_and_the_first_is_unchanged():
    ext = _lib.all_symbols(_lib_ext.EXT_HEADER_TABLES)
    assert not set(ext) & set(_lib.all_symbols())
    assert len(_lib.all_symbols()) == 134
    lib = _lib.load()
    assert lib.fsnp_abi_version() == 13 == _lib.ABI_VERSION
    for name, (res, args) in ext.items():
        fn = getattr(lib, name)                  # load() bound them on the one CDLL
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    # the extension header reaches fsnp.h, fsnp.h does not reach it; and the build hash sees it
    with open(os.path.join(ROOT, "include", "fsnp.h")) as f:
        assert "ext/" not in f.read()
    assert os.path.realpath(os.path.join(ROOT, "include", "ext", "fsnp_windowed.h")) in {os.path.realpath(h) for h in _build._headers()}
    assert {"windowed.hip", "fsnp_windowed_abi.hip"} <= set(_build._sources())


def test_header_is_plain_c_and_links_from_c(tmp_path):
    """include/ext/fsnp_windowed.h compiles as C99 with -Wall -Werror -pedantic and tests/c_abi/windowed_check.c gets -1 / K from
    fsnp_window_count."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    _lib.load()
    exe = tmp_path / "windowed_check"
    libdir = os.path.dirname(_build.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c_abi", "windowed_check.c"), "-o", str(exe), "-L", libdir, "-lfsnp_hip", "-Wl,-rpath," + libdir]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "bad=-1,-1,-1,-1 K=3,1,2,1 null rc=1" in run.stdout and "fsnp_enhance_wave_windowed" in run.stdout


# ------------------------------------------------------------------------------------------------ Python refusals
@pytest.mark.parametrize("cls,args", [(FullSubNet_Plus, DEFAULT_MODEL_ARGS), (FullSubNet, FULLSUBNET_MODEL_ARGS)], ids=["plus", "fullsubnet"])
def test_python_refusals_come_before_any_gpu(cls, args):
    m = cls(**args)
    wav = torch.zeros(1, 10000)                                        # a CPU tensor: the last refusal of all
    for kw, what in (({"window": 4096.0, "overlap": 1024}, "window must be an integer"),
                     ({"window": 4096, "overlap": 1024.5}, "overlap must be an integer"),
                     ({"window": True, "overlap": 1024}, "window must be an integer"),
                     ({"window": 4096, "overlap": 255}, r"overlap 255 outside \[n_fft / 2, window / 2\] = \[256, 2048\]"),
                     ({"window": 4096, "overlap": 2049}, "overlap 2049 outside"),
                     ({"window": 4097, "overlap": 2049}, "overlap 2049 outside"),
                     ({"window": 4096, "overlap": 1024, "max_batch": 0}, "max_batch 0 < 1"),
                     ({"window": 4096, "overlap": 1024, "max_batch": 2.0}, "max_batch must be an integer"),
                     ({"window": 4096, "overlap": 1024, "out_format": "s24"}, "out_format")):
        with pytest.raises(ValueError, match=what):
            m.enhance_wave_windowed(wav, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.enhance_wave_windowed(wav, 4096, 1024)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.enhance_wave_windowed(wav, window=np.int64(4096), overlap=np.int32(2048), max_batch=1)      # integers of any kind are fine
    assert m._hip.handle is None                                       # nothing was created on the way
