"""ctypes binding of the headers under include/<dir>/: the registries behind _lib's own, built by the rules of _lib.HEADER_TABLES.

_lib's own registry mirrors include/*.h and is closed (its tables and prototype count are pinned by tests/test_host_abi_signatures.py);
an entry point added after that gets its header under include/ext/ and its table here.  Same library, same ABI version: bind() types
these symbols on the CDLL that _lib.load() made, and load() calls it, so a caller sees one library object.

include/ext/ is closed in its turn (tests/test_host_windowed.py pins it to one header); a header added after that goes into a directory
of its own kind under include/ - session headers under include/session/ - and its table into SUBDIR_HEADER_TABLES, which
tests/test_host_window_stream.py compares with what is on disk under every include/<dir>/ other than ext/, pinning no count."""
import ctypes

from ._lib import c_i32, c_i64, c_vp

_WINDOWED_CALL = (c_i32, [c_vp, c_vp, c_i32, c_i64, c_i64, c_vp, c_i32, c_i64, c_i64, ctypes.POINTER(c_i32), c_i32, c_i32, c_i32, c_i32, c_i32,
                          c_vp, c_vp])

# every symbol include/ext/fsnp_windowed.h declares (a long recording in overlapping windows, cross-faded on the device)
WINDOWED_SYMBOLS = {
    "fsnp_window_count": (c_i64, [c_i64, c_i32, c_i32]),
    "fsnp_enhance_wave_windowed": _WINDOWED_CALL,
    "fsnp_debug_window_roundtrip": _WINDOWED_CALL,
}

# include/<header> -> the table that mirrors it; tests/test_host_windowed.py compares them type by type
EXT_HEADER_TABLES = {"ext/fsnp_windowed.h": WINDOWED_SYMBOLS}


_WINDOW_STREAM_CREATE = (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, ctypes.POINTER(c_vp)])

# every symbol include/session/fsnp_window_stream.h declares (window sessions: live audio through either model in cross-faded windows)
WINDOW_STREAM_SYMBOLS = {
    "fsnp_window_stream_plan": (c_i32, [c_i64, c_i64, c_i32, c_i32, ctypes.POINTER(c_i64), ctypes.POINTER(c_i64)]),
    "fsnp_window_stream_create": _WINDOW_STREAM_CREATE,
    "fsnp_window_stream_destroy": (None, [c_vp]),
    "fsnp_window_stream_push_pcm": (c_i32, [c_vp, c_vp, c_i32, c_i64, c_i64, ctypes.POINTER(c_i32), c_vp, c_i32, c_i64, c_i64, c_i32, c_vp, c_vp]),
    "fsnp_window_stream_finish_pcm": (c_i32, [c_vp, ctypes.POINTER(c_i32), c_i32, c_vp, c_i32, c_i64, c_i64, c_vp, c_vp]),
    "fsnp_window_stream_reset": (c_i32, [c_vp, ctypes.POINTER(c_i32), c_i32, c_vp]),
    "fsnp_window_stream_delay": (c_i32, [c_vp]),
    "fsnp_window_stream_samples": (c_i32, [c_vp, c_i32, ctypes.POINTER(c_i64)]),
    "fsnp_window_stream_state_bytes": (c_i64, [c_vp]),
    "fsnp_window_stream_get_state": (c_i32, [c_vp, c_i32, c_vp, c_vp]),
    "fsnp_window_stream_set_state": (c_i32, [c_vp, c_i32, c_vp, c_vp]),
    "fsnp_debug_window_stream_create_copy": _WINDOW_STREAM_CREATE,
}

# include/<dir>/<header> for every <dir> but ext/ -> the table that mirrors it
SUBDIR_HEADER_TABLES = {"session/fsnp_window_stream.h": WINDOW_STREAM_SYMBOLS}


def bind(lib):
    """Type every entry point of both mappings on `lib`; AttributeError if the library does not export one."""
    from ._lib import all_symbols
    for name, (res, args) in all_symbols({**EXT_HEADER_TABLES, **SUBDIR_HEADER_TABLES}).items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib
