"""The argument checks of the two calls of the cached rectangles need no GPU: a null context and a
null result are refused before anything touches the device."""
import ctypes


def test_rect_cache_calls_refuse_null_arguments(arvx):
    lib = arvx.load_library()
    n = ctypes.c_int64(7)
    assert lib.arvx_ctx_set_rect_cache_limit(None, 0) == 1  # ARVX_ERR_INVALID
    assert b"null" in lib.arvx_last_error()
    assert lib.arvx_ctx_set_rect_cache_limit(None, 1 << 30) == 1
    assert lib.arvx_selftest_rect_cache(None, ctypes.byref(n)) == 1
    assert b"null" in lib.arvx_last_error()
    assert n.value == 7  # (a refused call writes nothing)


def test_rect_cache_names(arvx):
    """The path bit is a new one, and the binding declares the calls' arguments."""
    bits = [getattr(arvx, k) for k in dir(arvx) if k.startswith("PATH_")]
    assert len(set(bits)) == len(bits) and all(b & (b - 1) == 0 for b in bits)
    assert arvx.PATH_RECT_BLOCKS in bits
    lib = arvx.load_library()
    assert lib.arvx_ctx_set_rect_cache_limit.argtypes[1] is ctypes.c_uint64
    assert {"arvx_ctx_set_rect_cache_limit", "arvx_selftest_rect_cache"} <= set(arvx.SYMBOLS)
