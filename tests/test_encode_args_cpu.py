"""CPU-side checks of the encode family's argument rules: every entry refuses a bad descriptor with the documented code, before anything
touches a device, and names ITSELF in the message (the entries share one check, csrc/codebook_encode.hip:encode_check)."""
import ctypes as C

import numpy as np
import pytest

# entry -> (levels it takes, seg_num values it refuses, its arguments after the descriptor: "in" is the map, "lw" the level blobs,
# "tau" the candidates' float thresholds, "p" any other device pointer, an int the 64-wide form's cin_total)
CAND = ("in", "p", "p", "p", "tau", "p", "p", "p")
ENTRIES = {
    "qv2x_codebook_encode_f32": (4, (3,), ("in", "lw", "p")),
    "qv2x_codebook_encode_f32in": (4, (3,), ("in", "lw", "p")),
    "qv2x_codebook_encode_wave_f32": (4, (3,), ("in", None, "lw", "p")),
    "qv2x_codebook_encode_listed_f32": (4, (3, 4), ("in", "lw", "p", "p", "p")),
    "qv2x_codebook_encode_span_f32": (3, (3, 4), ("in", "lw", "p", "p", "p")),
    "qv2x_codebook_encode64_f32": (4, (3,), (64, "in", "lw", "p")),
    "qv2x_codebook_encode64_f32in": (4, (3,), (64, "in", "lw", "p")),
    "qv2x_codebook_encode_candidates_i8": (3, (3, 2), CAND),
    "qv2x_codebook_encode_candidates_seg_i8": (3, (3, 4), CAND),
    "qv2x_codebook_encode_candidates_span_i8": (3, (3, 4), CAND),
    "qv2x_codebook_encode_collapsed_f32": (3, (3, 2), ("in", "p", "p", "p", "p")),
}


@pytest.fixture(scope="module")
def l():
    from quantv2x_amd import build, lib
    build.build()
    return lib.load()


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_entry_refuses_bad_descriptors_in_its_own_name(l, name):
    from quantv2x_amd import lib
    max_levels, bad_segs, spec = ENTRIES[name]
    buf = np.zeros(4096, np.uint8)                                    # host memory: every check below runs before a launch
    base = (buf.ctypes.data + 15) & ~15
    lw, tau = (C.c_void_p * 5)(*[base + 256 * i for i in range(5)]), (C.c_float * 9)()

    def desc(**kw):
        d = lib.EncodeDesc()
        d.n, d.h, d.w, d.levels, d.kc, d.in_zx, d.in_delta, d.segs = 1, 4, 4, 3, 64, 0, 0.1, 1
        for k, v in kw.items():
            setattr(d, k, v)
        return C.byref(d)

    def call(d, in_ptr=base):
        args = [{"in": C.c_void_p(in_ptr), "lw": lw, "tau": tau, "p": C.c_void_p(base), None: None}.get(a, a) for a in spec]
        rc = getattr(l, name)(d, *args, None)
        msg = l.qv2x_last_error().decode()
        assert msg.startswith(name + ":"), (rc, msg)
        return rc, msg

    rc, msg = call(None)
    assert rc == -1 and "null" in msg
    rc, msg = call(desc(kc=100))
    assert rc == -1 and "dict_size" in msg
    rc, msg = call(desc(levels=max_levels + 1))
    assert rc == -1 and "levels" in msg
    rc, msg = call(desc(), in_ptr=base + 1)
    assert rc == -2 and "aligned" in msg
    for segs in bad_segs:
        rc, msg = call(desc(segs=segs))
        assert rc == -1 and "seg_num" in msg, (segs, msg)
