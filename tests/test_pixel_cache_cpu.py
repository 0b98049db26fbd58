"""The argument checks of the calls of the cached pixels need no GPU: a null context and a null
result are refused before anything touches the device."""
import ctypes


def test_pixel_cache_calls_refuse_null_arguments(arvx):
    lib = arvx.load_library()
    n = ctypes.c_int64(7)
    words = (ctypes.c_uint64 * 2)(5, 5)
    assert lib.arvx_ctx_set_pixel_cache_limit(None, 0) == 1  # ARVX_ERR_INVALID
    assert b"null" in lib.arvx_last_error()
    assert lib.arvx_ctx_set_pixel_cache_limit(None, 6 << 30) == 1
    assert lib.arvx_selftest_pixel_cache(None, ctypes.byref(n)) == 1
    assert b"null" in lib.arvx_last_error()
    assert lib.arvx_pixel_cache_views(None, words, 2) == 1
    assert b"null" in lib.arvx_last_error()
    assert n.value == 7 and list(words) == [5, 5]  # (a refused call writes nothing)


def test_pixel_cache_names(arvx):
    """The path bit is a new one, and the binding declares the calls' arguments."""
    bits = [getattr(arvx, k) for k in dir(arvx) if k.startswith("PATH_")]
    assert len(set(bits)) == len(bits) and all(b & (b - 1) == 0 for b in bits)
    assert arvx.PATH_PIXEL_TABLE in bits
    lib = arvx.load_library()
    assert lib.arvx_ctx_set_pixel_cache_limit.argtypes[1] is ctypes.c_uint64
    assert lib.arvx_pixel_cache_views.argtypes[2] is ctypes.c_int
    assert {"arvx_ctx_set_pixel_cache_limit", "arvx_pixel_cache_views",
            "arvx_selftest_pixel_cache"} <= set(arvx.SYMBOLS)
