"""Host tests of the window sessions (include/session/fsnp_window_stream.h): the schedule by brute force against the windowed call's
float restatement, fsnp_window_stream_plan, the registry of the headers under include/<dir>/ against what is on disk, the header as
plain C, and the Python refusals that need no GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import fullsubnet_plus_amd
from fullsubnet_plus_amd import FullSubNet, FullSubNet_Plus, _build, _lib, _lib_ext
from fullsubnet_plus_amd.synthetic import DEFAULT_MODEL_ARGS, FULLSUBNET_MODEL_ARGS
from tests._window_stream_util import SlotSim, random_blocks
from tests._windowed_util import merge, window_plan
from tests.test_host_abi_signatures import mismatches, parse_prototypes, table_classes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF = 256                                   # n_fft / 2 of the default geometry: the smallest overlap


def _overlaps(W):
    return sorted(set(range(HALF, W // 2 + 1, 37)) | {W // 2})


# ------------------------------------------------------------------------------------------------ the schedule
@pytest.mark.parametrize("W", [1024, 1500, 4096])
def test_schedule_by_brute_force(W):
    """Random chunkings (blocks of 1 ... 3 W, idle pushes included) of random clips on identity windows: SlotSim asserts that every
    output is available when due, that pending never exceeds S and that finish has at most one window left, of more than V samples
    or the whole clip; here: the windows the pushes ran are the plan's full windows, fsnp_window_stream_plan agrees at every push,
    and pushes + finish without the first W samples are merge() of the plan's windows."""
    lib = _lib.load()
    rng = np.random.default_rng(W)
    clips = 0
    for V in _overlaps(W):
        S = W - V
        # lengths: random, and the edges - one window exactly, k S + W exactly, one sample either side, a clip below one window
        lengths = [int(rng.integers(HALF + 1, 4 * W)), W, 2 * S + W, 2 * S + W + 1, 2 * S + W - 1, S + V + 1, int(rng.integers(HALF + 1, W))]
        for L in lengths:
            x = rng.standard_normal(L)
            sim = SlotSim(W, V)
            got, held = [], 0
            for c in random_blocks(rng, L, int(rng.choice([61, S, 3 * W]))):
                got.append(sim.push(x[held:held + c]))
                first, num = fullsubnet_plus_amd.window_stream_plan(held, c, W, V)
                assert (first, num) == sim.per_push[-1], (W, V, L, held, c)
                held += c
            got.append(sim.finish())
            plan = window_plan(L, W, V)
            assert sim.ran == plan, (W, V, L)
            total = np.concatenate(got)
            assert len(total) == L + W and not total[:W].any(), (W, V, L)      # exact zeros before the delay
            assert np.array_equal(total[W:], merge([x[a:a + n] for a, n in plan], L, W, V)), (W, V, L)
            assert np.array_equal(total[W:], x)                                                  # identity windows: the clip itself
            clips += 1
    assert clips >= 50
    c_first, c_num = fullsubnet_plus_amd.window_stream_plan(2 ** 40, 2 ** 33, 4096, 1024)
    assert c_first == (2 ** 40 - 4096) // 3072 + 1 and c_num == (2 ** 40 + 2 ** 33 - 4096) // 3072 + 1 - c_first
    assert lib.fsnp_window_stream_plan.restype is _lib.c_i32


def test_plan_refuses_what_needs_no_handle():
    import ctypes
    lib = _lib.load()
    first, num = ctypes.c_int64(-7), ctypes.c_int64(-7)
    for bad in ((0, 1, 1, 1), (0, 1, 4096, 0), (0, 1, 4096, 2049), (0, 1, 4096, -5), (-1, 1, 4096, 1024), (0, -1, 4096, 1024), (0, 1, -8, 1)):
        assert lib.fsnp_window_stream_plan(*bad, ctypes.byref(first), ctypes.byref(num)) == -1, bad
        with pytest.raises(ValueError, match="window_stream_plan"):
            fullsubnet_plus_amd.window_stream_plan(*bad)
    assert lib.fsnp_window_stream_plan(0, 1, 4096, 1024, None, ctypes.byref(num)) == -1
    assert lib.fsnp_window_stream_plan(0, 1, 4096, 1024, ctypes.byref(first), None) == -1
    assert (first.value, num.value) == (-7, -7)                                      # a refusal writes nothing
    assert fullsubnet_plus_amd.window_stream_plan(0, 2, 2, 1) == (0, 1) and fullsubnet_plus_amd.window_stream_plan(np.int64(2), np.int32(5), 2, 1) == (1, 5)


def test_float32_restatement_follows_the_librarys_schedule_and_merges_like_the_windowed_call():
    """SlotSim in float32 with a window function that is not the identity, driven by the LIBRARY's schedule: at every push the windows
    that run are the ones fsnp_window_stream_plan names for the slot's count (a push asked to run anything else fails here), and the
    samples that come out are merge()'s, bit for bit, whatever the chunking (one fused multiply-add per overlapped sample)."""
    rng = np.random.default_rng(3)
    W, V, L = 1024, 293, 4000
    S = W - V
    x = rng.standard_normal(L).astype(np.float32)

    def enhance(w):
        return (np.asarray(w, dtype=np.float32) * np.float32(0.7) + np.float32(0.01) * np.float32(len(w))).astype(np.float32)
    want = merge([enhance(x[a:a + n]) for a, n in window_plan(L, W, V)], L, W, V, np.float32)
    for largest in (1, 97, 3000):
        sim = SlotSim(W, V, enhance, np.float32)
        got, held = [], 0
        for c in random_blocks(rng, L, largest) if largest > 1 else [1] * L:
            first, num = fullsubnet_plus_amd.window_stream_plan(held, c, W, V)
            ran = len(sim.ran)
            got.append(sim.push(x[held:held + c]))
            assert sim.ran[ran:] == [(k * S, W) for k in range(first, first + num)], (largest, held, c)
            held += c
        total = np.concatenate(got + [sim.finish()])
        assert total.dtype == np.float32 and np.array_equal(total[W:], want), largest


# ------------------------------------------------------------------------------------------------ the registries
def test_headers_in_subdirectories_match_their_tables_type_by_type():
    """Every header under every include/<dir>/ other than ext/ has a table in _lib_ext.SUBDIR_HEADER_TABLES and the other way round,
    and every table matches its header's prototypes type by type.  No count is pinned: the next header needs no further registry."""
    include = os.path.join(ROOT, "include")
    on_disk = {f"{d}/{f}" for d in os.listdir(include) if d != "ext" and os.path.isdir(os.path.join(include, d))
               for f in os.listdir(os.path.join(include, d)) if f.endswith(".h")}
    assert on_disk == set(_lib_ext.SUBDIR_HEADER_TABLES) and "session/fsnp_window_stream.h" in on_disk
    for header, table in _lib_ext.SUBDIR_HEADER_TABLES.items():
        with open(os.path.join(include, header)) as f:
            text = f.read()
        declared = parse_prototypes(text)
        assert declared and mismatches(declared, table_classes(table)) == [], header
        assert os.path.realpath(os.path.join(include, header)) in {os.path.realpath(h) for h in _build._headers()}, header
    names = set(_lib_ext.WINDOW_STREAM_SYMBOLS)
    assert {"fsnp_window_stream_" + n for n in ("plan", "create", "destroy", "push_pcm", "finish_pcm", "reset", "delay", "samples",
                                                "state_bytes", "get_state", "set_state")} | {"fsnp_debug_window_stream_create_copy"} == names


def test_the_first_two_registries_are_unchanged_and_all_three_share_no_name():
    first, ext, sub = _lib.all_symbols(), _lib.all_symbols(_lib_ext.EXT_HEADER_TABLES), _lib.all_symbols(_lib_ext.SUBDIR_HEADER_TABLES)
    assert len(first) == 134 and len(_lib.HEADER_TABLES) == 12 and len({id(t) for t in _lib.HEADER_TABLES.values()}) == 11
    assert set(_lib_ext.EXT_HEADER_TABLES) == {"ext/fsnp_windowed.h"} and len(ext) == 3
    assert not set(first) & set(ext) and not set(first) & set(sub) and not set(ext) & set(sub)
    lib = _lib.load()
    assert lib.fsnp_abi_version() == 13 == _lib.ABI_VERSION
    for name, (res, args) in {**ext, **sub}.items():
        fn = getattr(lib, name)                  # load() bound both mappings on the one CDLL
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    # the session header reaches fsnp.h and the windowed header, neither reaches it
    with open(os.path.join(ROOT, "include", "session", "fsnp_window_stream.h")) as f:
        text = f.read()
    assert '#include "../fsnp.h"' in text and '#include "../ext/fsnp_windowed.h"' in text
    for other in ("fsnp.h", os.path.join("ext", "fsnp_windowed.h")):
        with open(os.path.join(ROOT, "include", other)) as f:
            assert "session/" not in f.read(), other
    assert {"window_stream.hip", "fsnp_window_stream_abi.hip"} <= set(_build._sources())


def test_header_is_plain_c_and_links_from_c(tmp_path):
    """include/session/fsnp_window_stream.h compiles as C99 with -Wall -Werror -pedantic and tests/c_abi/window_stream_check.c gets the
    plan's numbers from fsnp_window_stream_plan."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    _lib.load()
    exe = tmp_path / "window_stream_check"
    libdir = os.path.dirname(_build.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c_abi", "window_stream_check.c"), "-o", str(exe), "-L", libdir, "-lfsnp_hip", "-Wl,-rpath," + libdir]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ok=0,0,0,0 bad=-1,-1,-1,-1 plan=0+0,0+1,1+2,2+0 delay=0 null rc=1" in run.stdout and "fsnp_window_stream_create" in run.stdout


# ------------------------------------------------------------------------------------------------ Python refusals
@pytest.mark.parametrize("cls,args", [(FullSubNet_Plus, DEFAULT_MODEL_ARGS), (FullSubNet, FULLSUBNET_MODEL_ARGS)], ids=["plus", "fullsubnet"])
def test_python_refusals_come_before_any_gpu(cls, args):
    m = cls(**args)
    for kw, what in (({"window": 4096.0, "overlap": 1024}, "window must be an integer"),
                     ({"window": 4096, "overlap": 1024.5}, "overlap must be an integer"),
                     ({"window": True, "overlap": 1024}, "window must be an integer"),
                     ({"window": 4096, "overlap": 255}, r"overlap 255 outside \[n_fft / 2, window / 2\] = \[256, 2048\]"),
                     ({"window": 4096, "overlap": 2049}, "overlap 2049 outside"),
                     ({"window": 4097, "overlap": 2049}, "overlap 2049 outside"),
                     ({"window": 4096, "overlap": 2048, "max_batch": 0}, "max_batch 0 < 1"),
                     ({"window": 4096, "overlap": 2048, "max_batch": 2.0}, "max_batch must be an integer"),
                     ({"window": 4096, "overlap": 2048, "max_samples": 0}, "max_samples 0 < 1"),
                     ({"window": 4096, "overlap": 2048, "max_samples": 160.0}, "max_samples must be an integer"),
                     ({"window": 4096, "overlap": 2048, "slots": 0}, "slots 0 < 1"),
                     ({"window": 4096, "overlap": 2048, "slots": "2"}, "slots must be an integer"),
                     ({"window": 4096, "overlap": 2048, "slots": 2 ** 31}, "slots 2147483648 is not an int32"),
                     ({"window": 4096, "overlap": 2048, "max_samples": 2 ** 40}, "max_samples 1099511627776 is not an int32")):
        with pytest.raises(ValueError, match=what):
            m.open_window_stream(**{"slots": 2, **kw})
    assert m._hip.handle is None                                       # nothing was created on the way
    # the three frame- and sample-fed openers of FullSubNet+ keep raising exactly as they do
    if cls is FullSubNet_Plus:
        for opener in (m.open_stream, m.open_wave_stream, m.open_spec_stream):
            with pytest.raises(NotImplementedError, match="FullSubNet\\+ cannot be streamed exactly"):
                opener(1)
        assert m._hip.handle is None


def test_push_and_finish_refuse_formats_before_the_session_is_touched():
    """out_format is checked first of all in push and finish: a session object without a C session behind it is enough to see it."""
    from fullsubnet_plus_amd.stream import WindowStream
    ws = WindowStream.__new__(WindowStream)
    ws._st = None
    wav = torch.zeros(2, 160)
    for call in (lambda f: ws.push(wav, out_format=f), lambda f: ws.finish(out_format=f)):
        with pytest.raises(ValueError, match="out_format 's16_peak' is none of None, 'f32', 's16' .a stream has no peak"):
            call("s16_peak")
        with pytest.raises(ValueError, match="out_format 's24'"):
            call("s24")
        with pytest.raises(RuntimeError, match="this stream is closed"):
            call("s16")
