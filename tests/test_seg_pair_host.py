"""pcadv_gather_seg_pair (the adversarial seg steps' packed input in one launch)
validates its two jobs on the host before any launch: no GPU needed.  Every
refusal is a non-zero return code with a message; nothing is launched (the
pointers below are made-up addresses no kernel ever sees)."""
import ctypes

import pytest

from adversarial_learning_on_pointclouds_amd import _lib


def _job(**kw):
    """A complete job over made-up addresses (never dereferenced on the host)."""
    a = lambda k: 0x100000 * k  # noqa: E731
    d = dict(src=a(1), n_src=5, npts=48, src_npts=50, order=a(2), cursor=a(3), B=2, src_lab=a(4),
             lab_width=1, src_seg=None, sigma=0.0, clip=0.05, seed=1, step=a(5), rng_row0=0)
    d.update(kw)
    return _lib.GatherJob(**d)


def _call(lib, gt, ng, C=16, pts=0x700000, cls=0x800000, seg=0x900000):
    P = lambda v: None if v is None else ctypes.c_void_p(v)  # noqa: E731
    return lib.pcadv_gather_seg_pair(None if gt is None else ctypes.byref(gt),
                                     None if ng is None else ctypes.byref(ng), C, P(pts), P(cls),
                                     P(seg), None)


GT = dict(src_seg=0x600000)


def test_symbol_is_exported_and_declared():
    lib = _lib.load()
    assert hasattr(lib, "pcadv_gather_seg_pair")
    import os
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "pcadv.h")).read()
    assert "int pcadv_gather_seg_pair(" in hdr


@pytest.mark.parametrize("field", ["src", "order", "cursor", "src_lab"])
@pytest.mark.parametrize("which", [0, 1])
def test_refuses_a_missing_job_field(field, which):
    lib = _lib.load()
    jobs = [_job(**GT), _job()]
    jobs[which] = _job(**dict(GT if which == 0 else {}, **{field: None}))
    assert _call(lib, *jobs) != 0
    assert b"bad arguments" in lib.pcadv_last_error()


def test_refuses_a_missing_job_or_output():
    lib = _lib.load()
    gt, ng = _job(**GT), _job()
    for kw in (dict(pts=None), dict(cls=None), dict(seg=None)):
        assert _call(lib, gt, ng, **kw) != 0
        assert b"missing" in lib.pcadv_last_error()
    assert _call(lib, None, ng) != 0 and _call(lib, gt, None) != 0


@pytest.mark.parametrize("kw, msg", [
    (dict(B=3), b"jobs differ"),          # unequal B
    (dict(npts=47), b"jobs differ"),      # unequal npts
])
def test_refuses_unequal_jobs(kw, msg):
    lib = _lib.load()
    assert _call(lib, _job(**GT), _job(**kw)) != 0
    assert msg in lib.pcadv_last_error()


@pytest.mark.parametrize("C", [0, 65, -1])
def test_refuses_class_counts_outside_1_to_64(C):
    lib = _lib.load()
    assert _call(lib, _job(**GT), _job(), C=C) != 0
    assert b"classes" in lib.pcadv_last_error()


def test_refuses_part_ids_on_the_wrong_job():
    lib = _lib.load()
    assert _call(lib, _job(), _job()) != 0            # a GT job without part ids
    assert b"part ids" in lib.pcadv_last_error()
    assert _call(lib, _job(**GT), _job(**GT)) != 0    # a no-GT job with part ids
    assert b"part ids" in lib.pcadv_last_error()


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("lw", [0, 2])
def test_refuses_a_label_width_other_than_one(which, lw):
    lib = _lib.load()
    jobs = [_job(**GT), _job()]
    jobs[which] = _job(**dict(GT if which == 0 else {}, lab_width=lw))
    assert _call(lib, *jobs) != 0
    assert b"lab_width" in lib.pcadv_last_error()


def test_refuses_a_jitter_without_clip():
    lib = _lib.load()
    assert _call(lib, _job(**GT), _job(sigma=0.01, clip=0.0)) != 0
    assert b"clip" in lib.pcadv_last_error()
