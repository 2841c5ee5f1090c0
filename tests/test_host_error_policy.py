"""fullsubnet_plus_amd/_policy.py: what forward, enhance_wave and the stream sessions' pushes do with the codes a launch reports
afterwards, driven by recording stubs: the exact call sequence of every case.  No GPU, no library."""
import pytest

from fullsubnet_plus_amd import _lib, _policy


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    monkeypatch.setattr(_lib, "last_error", lambda: "stub")          # (_lib.check asks the library for the text)


def _enqueue(rcs):
    calls, rcs = [], list(rcs)

    def enqueue():
        calls.append("enqueue")
        return rcs.pop(0)
    return calls, enqueue, lambda: calls.append("noticed")


@pytest.mark.parametrize("rcs,want", [((0,), ["enqueue"]), ((6, 0), ["enqueue", "noticed", "enqueue"])])
def test_enqueue_passes(rcs, want):
    calls, enqueue, noticed = _enqueue(rcs)
    assert _policy.enqueue_retrying_stale(enqueue, noticed, "fsnp_x") is None
    assert calls == want


@pytest.mark.parametrize("rcs,code,want", [((6, 6), 6, ["enqueue", "noticed", "enqueue"]), ((2,), 2, ["enqueue"])])
def test_enqueue_raises(rcs, code, want):
    calls, enqueue, noticed = _enqueue(rcs)
    with pytest.raises(_lib.FsnpError, match="^fsnp_x") as e:
        _policy.enqueue_retrying_stale(enqueue, noticed, "fsnp_x")
    assert e.value.code == code and calls == want


class _Stubs:
    """run() returns "out1", "out2", ...; wait_and_poll() returns the given codes in turn; everything records its name."""

    def __init__(self, polls=(), state=True, fallback=False):
        self.calls, self.polls = [], list(polls)
        self.kw = {"wait_and_poll": self.wait_and_poll, "repack": lambda: self.calls.append("repack")}
        if state:
            self.kw.update(save=lambda: self.calls.append("save"), restore=lambda: self.calls.append("restore"))
        if fallback:
            self.kw["fallback"] = self.fallback

    def run(self):
        self.calls.append("run")
        return f"out{self.calls.count('run')}"

    def wait_and_poll(self):
        self.calls.append("poll")
        return self.polls.pop(0)

    def fallback(self, run):
        assert run == self.run
        self.calls.append("fallback")
        return "fallback's"


def test_deferred_runs_and_calls_nothing_else():
    s = _Stubs(fallback=True)
    assert _policy.run_checked(s.run, "fsnp_x", sync=False, **s.kw) == "out1"
    assert s.calls == ["run"]


@pytest.mark.parametrize("state", [True, False])
def test_sync_clean(state):
    s = _Stubs([0], state, fallback=True)
    assert _policy.run_checked(s.run, "fsnp_x", sync=True, **s.kw) == "out1"
    assert s.calls == ["save"] * state + ["run", "poll"]


@pytest.mark.parametrize("fallback", [True, False])
def test_sync_stale_weights_restore_repack_and_run_again(fallback):
    s = _Stubs([6, 0], fallback=fallback)
    assert _policy.run_checked(s.run, "fsnp_x", sync=True, **s.kw) == "out2"
    assert s.calls == ["save", "run", "poll", "restore", "repack", "run", "poll"]
    s = _Stubs([6, 0], state=False, fallback=fallback)
    assert _policy.run_checked(s.run, "fsnp_x", sync=True, **s.kw) == "out2"
    assert s.calls == ["run", "poll", "repack", "run", "poll"]


def test_sync_stale_weights_twice_raises():
    s = _Stubs([6, 6], fallback=True)
    with pytest.raises(_lib.FsnpError, match="^fsnp_x") as e:
        _policy.run_checked(s.run, "fsnp_x", sync=True, **s.kw)
    assert e.value.code == 6 and s.calls == ["save", "run", "poll", "restore", "repack", "run", "poll"]


@pytest.mark.parametrize("code", [5, 7])
def test_sync_timeout_or_failed_verification(code):
    s = _Stubs([code], fallback=True)
    assert _policy.run_checked(s.run, "fsnp_x", sync=True, **s.kw) == "fallback's"
    assert s.calls == ["save", "run", "poll", "fallback"]
    s = _Stubs([code])
    with pytest.raises(_lib.FsnpError, match="^fsnp_x failed") as e:
        _policy.run_checked(s.run, "fsnp_x", sync=True, **s.kw)
    assert e.value.code == code and s.calls == ["save", "run", "poll"]
