"""CPU: dwt_amd.View (ctypes) against the dwtx_view struct of include/dwtx.h — size, field names and order — and the
meaning of a View that fills only the first eight fields: channel_stride 0, interleaved pixels, as before the field."""
import ctypes as C
import os
import re

import dwt_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CTYPES = {"void *": C.c_void_p, "int": C.c_int, "size_t": C.c_size_t}


def header_fields():
    """[(type, name)] of `typedef struct dwtx_view { ... } dwtx_view;`, comments stripped."""
    text = open(os.path.join(ROOT, "include", "dwtx.h")).read()
    body = re.search(r"typedef\s+struct\s+dwtx_view\s*\{(.*?)\}\s*dwtx_view\s*;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            m = re.fullmatch(r"(void\s*\*|int|size_t)\s*(\w+)", decl)
            assert m, decl
            out.append((re.sub(r"\s+", " ", m.group(1)).replace("void*", "void *"), m.group(2)))
    return out


def test_view_matches_the_header():
    fields = header_fields()
    assert [name for _, name in fields] == [name for name, _ in dwt_amd.View._fields_]
    assert [CTYPES[t] for t, _ in fields] == [t for _, t in dwt_amd.View._fields_]
    assert fields[-1] == ("size_t", "channel_stride")

    class Mirror(C.Structure):   # the C compiler's layout of the header's declaration
        _fields_ = [(name, CTYPES[t]) for t, name in fields]

    assert C.sizeof(dwt_amd.View) == C.sizeof(Mirror) == 56
    for name, _ in Mirror._fields_:
        assert getattr(dwt_amd.View, name).offset == getattr(Mirror, name).offset, name


def test_eight_positional_values_mean_interleaved():
    v = dwt_amd.View(0x1000, 1, 3, 255, 4, 900, 216, 61200)
    assert v.channel_stride == 0
    assert (v.dev, v.sample_bytes, v.channels, v.maxval, v.cols, v.row_pitch, v.image_stride, v.band_stride) == \
        (0x1000, 1, 3, 255, 4, 900, 216, 61200)
