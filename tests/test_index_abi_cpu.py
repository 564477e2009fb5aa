"""CPU: what the appearance index's C ABI decides before it touches a device.  A configuration outside its ranges is
RTMODT_E_INVALID with nothing allocated (so the answer is the same on a machine without a GPU), the defaults are a valid
configuration, and a create on a device ordinal that cannot exist fails at ``hipSetDevice`` inside the shared open
(``csrc/handle_host.h``) and leaves a Python object that closes without a sound."""
import ctypes as C
import gc

import pytest

NO_DEVICE = 1 << 20


def test_default_cfg_is_the_documented_one(pkg):
    cfg = pkg._ffi.IndexCfg()
    pkg._ffi.lib().rtmodt_index_default_cfg(C.byref(cfg))
    assert (cfg.device, cfg.dim, cfg.capacity, cfg.max_queries, cfg.max_k, cfg.max_add, cfg.chunk_rows) == (0, 512, 1 << 20, 64, 64, 4096, 0)


@pytest.mark.parametrize("kw", [dict(dim=0), dict(dim=96), dict(dim=576), dict(capacity=0), dict(capacity=(1 << 22) + 1), dict(max_queries=0),
                                dict(max_queries=65), dict(max_k=0), dict(max_k=65), dict(max_add=0), dict(max_add=65537), dict(chunk_rows=-64),
                                dict(chunk_rows=96), dict(capacity=16385, chunk_rows=64)], ids=str)
def test_configuration_out_of_range_is_refused_before_any_device_call(pkg, kw):
    L = pkg._ffi.lib()
    cfg = pkg._ffi.IndexCfg()
    L.rtmodt_index_default_cfg(C.byref(cfg))
    cfg.device = NO_DEVICE                                      # a valid configuration would fail at hipSetDevice: these never get there
    for k, v in kw.items():
        setattr(cfg, k, v)
    h = C.c_void_p()
    assert L.rtmodt_index_create(C.byref(cfg), C.byref(h)) == pkg._ffi.E_INVALID and not h.value
    assert b"index" in L.rtmodt_last_error()


def test_create_on_a_device_that_cannot_exist(pkg):
    E = pkg._ffi.RtmodtError
    shell = None
    with pytest.raises(E) as info:
        try:
            pkg.tracking.AppearanceIndex(64, 100, device=NO_DEVICE)
        except E as e:
            tb = e.__traceback__
            while tb is not None:
                me = tb.tb_frame.f_locals.get("self")
                if isinstance(me, pkg._ffi.Handle):
                    shell = me
                tb = tb.tb_next
            raise
    assert info.value.code == pkg._ffi.E_HIP and "hipSetDevice" in info.value.msg
    assert shell is not None and not getattr(shell, "_h", None)
    shell.close()
    shell.close()
    del shell, info
    gc.collect()


def test_null_handles_are_refused_and_destroy_takes_null(pkg):
    L = pkg._ffi.lib()
    L.rtmodt_index_destroy(None)
    n = C.c_int64(0)
    assert L.rtmodt_index_forget(None, None, 0, C.byref(n)) == pkg._ffi.E_INVALID
    assert L.rtmodt_index_search(None, None, 0, None, 1, None, None) == pkg._ffi.E_INVALID
    assert L.rtmodt_index_create(None, None) == pkg._ffi.E_INVALID
