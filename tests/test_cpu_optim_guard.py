"""CPU-side checks of the optimizer tail's non-finite guard (toist_opt_finish_norm_guarded): the entry point is exported, refuses bad veto tables
with an error code before anything is launched, and the three words it writes sit where toist_amd.optim.device_state() reads them."""
import ctypes


def test_library_exports_the_guarded_finish_norm():
    from toist_amd import _lib
    assert "toist_opt_finish_norm_guarded" in _lib.exported_symbols()
    assert hasattr(_lib.lib(), "toist_opt_finish_norm_guarded")


def test_bad_veto_tables_return_error_codes_without_a_gpu():
    """More than 8 words of a kind, or a NULL table with a positive count: TOIST_EINVAL and a message, no launch (the pointers are never read)."""
    from toist_amd import _lib
    fn = _lib.lib().toist_opt_finish_norm_guarded
    partial = (ctypes.c_float * 4)()
    state = (ctypes.c_uint8 * 32)()
    table = (ctypes.c_int64 * 16)()
    p, s, t = (ctypes.cast(x, ctypes.c_void_p) for x in (partial, state, table))
    assert fn(p, 4, 0.1, 0.9, 0.999, s, t, 9, None, 0, None) == -1 and "at most 8" in _lib.last_error()
    assert fn(p, 4, 0.1, 0.9, 0.999, s, None, 0, t, 9, None) == -1 and "at most 8" in _lib.last_error()
    assert fn(p, 4, 0.1, 0.9, 0.999, s, t, -1, None, 0, None) == -1
    assert fn(p, 4, 0.1, 0.9, 0.999, s, None, 1, None, 0, None) == -1 and "NULL veto table" in _lib.last_error()
    assert fn(p, 4, 0.1, 0.9, 0.999, s, None, 0, None, 3, None) == -1 and "NULL veto table" in _lib.last_error()
    assert fn(None, 4, 0.1, 0.9, 0.999, s, None, 0, None, 0, None) == -1 and "bad args" in _lib.last_error()
    assert fn(p, 4, 0.1, 1.0, 0.999, s, None, 0, None, 0, None) == -1 and "betas" in _lib.last_error()
    assert bytes(state) == bytes(32)          # nothing was written


def test_guard_words_sit_behind_the_step_count(tmp_path):
    from abi_probe import c_values
    got = c_values(tmp_path, ["sizeof(toist_opt_state)", "offsetof(toist_opt_state, step)", "offsetof(toist_opt_state, skipped)",
                              "offsetof(toist_opt_state, skipped_total)", "offsetof(toist_opt_state, veto_mask)", "TOIST_OPT_MAX_VETO"])
    assert got == [32, 16, 20, 24, 28, 8]
    from toist_amd.optim import FusedClipAdamWEMA
    assert FusedClipAdamWEMA.MAX_VETO == 8
