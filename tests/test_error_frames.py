"""An ECM2Error must not keep its caller's frame alive: the Python mirror raises it without holding
it in a local of a frame of its own traceback, so that once the caller has handled it, the caller's
locals (forms, device tensors, captured graphs) are released by reference counting at once -- not
by some later cyclic collection, which may fall inside a stream capture where the finalizers'
synchronising calls are illegal."""
import gc
import weakref

import pytest

import ecm2_amd as E


class _Token:
    pass


def _caller():
    tok = _Token()
    ref = weakref.ref(tok)
    with pytest.raises(E.ECM2Error):
        E.Mesh("/nonexistent/mesh/file.mesh")   # ecm2_mesh_read -> ECM2_ERR_IO -> _check raises
    return ref


def test_handled_error_releases_the_callers_frame_without_gc():
    E.load_library()   # (the first load imports torch, which runs under whatever frames called it)
    was = gc.isenabled()
    gc.disable()
    try:
        ref = _caller()
        assert ref() is None, "the handled ECM2Error still holds its caller's frame (a reference cycle)"
    finally:
        if was:
            gc.enable()


def test_error_carries_its_code():
    with pytest.raises(E.ECM2Error) as ei:
        E.Mesh("/nonexistent/mesh/file.mesh")
    assert ei.value.code == 4 and "ecm2 error 4" in str(ei.value)   # ECM2_ERR_IO
