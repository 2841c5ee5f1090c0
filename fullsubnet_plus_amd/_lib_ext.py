"""ctypes binding of the extension headers include/ext/*.h: the second registry, built by the rules of _lib.HEADER_TABLES.

_lib's own registry mirrors include/*.h and is closed (its tables and prototype count are pinned by tests/test_host_abi_signatures.py);
an entry point added after that gets its header under include/ext/ and its table here.  Same library, same ABI version: bind() types
these symbols on the CDLL that _lib.load() made, and load() calls it, so a caller sees one library object."""
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


def bind(lib):
    """Type every entry point of the extension headers on `lib`; AttributeError if the library does not export one."""
    from ._lib import all_symbols
    for name, (res, args) in all_symbols(EXT_HEADER_TABLES).items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib
