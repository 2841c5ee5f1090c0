"""The one error policy of every call that enqueues device work: forward, enhance, enhance_wave and the stream sessions' pushes.

A launch can report afterwards a timed-out exchange (_lib.ERR_TIMEOUT), weights that were edited through .data since they were packed
(_lib.ERR_STALE_WEIGHTS) or an exchange that failed verification (_lib.ERR_VERIFY); a LATER call on the handle is told.  Plain
functions over callables - no torch, no library - so tests/test_host_error_policy.py drives them with stubs."""
from . import _lib


def enqueue_retrying_stale(enqueue, noticed, what):
    """enqueue() -> rc enqueues one library call.  ERR_STALE_WEIGHTS from it is the weight watch's verdict on an EARLIER call: noticed()
    (the model warns and re-packs), then this call once more.  Whatever else is not 0 raises _lib.FsnpError."""
    rc = enqueue()
    if rc == _lib.ERR_STALE_WEIGHTS:
        noticed()
        rc = enqueue()
    _lib.check(rc, what)


def run_checked(run, what, *, sync, wait_and_poll, repack, save=None, restore=None, fallback=None):
    """run() -> out under the model's error_check.  "deferred" (sync=False): run() and nothing else.  "sync": wait_and_poll() -> rc
    waits for run()'s launches and polls the handle, so a result that is returned is never silently invalid:
      ERR_STALE_WEIGHTS  run() ran on the old weights: restore() (a session's states as save() kept them in front of run()), repack(),
                         and run() once more;
      any other code     fallback(run) where there is one (the model: the one-tile-per-CU kernel), FsnpError otherwise."""
    if not sync:
        return run()
    if save is not None:
        save()
    out = run()
    rc = wait_and_poll()
    if rc == _lib.ERR_STALE_WEIGHTS:
        if restore is not None:
            restore()
        repack()
        out = run()
        _lib.check(wait_and_poll(), f"{what} (after re-packing the weights)")
    elif rc != 0 and fallback is not None:
        return fallback(run)
    else:
        _lib.check(rc, what)
    return out
