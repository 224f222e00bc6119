"""The drop-in boundary, checked against the reference's own declarations (no reference code runs).

1. Every class / struct / enum / member that simian-spacemonkey_amd/host/gluvv_compat.h declares is
   looked up in the reference's MetaVolume.h, TLUT.h, gluvv.h and gluvvPrimitive.h and must carry the
   same type / return type / parameter types / constness there (compat may declare a subset, never
   something the reference lacks); enumerators must match in order.  The reference's declarations are
   oracle/_ref/reference_decls.json, which oracle/Makefile writes with oracle/header_decls.py (the parser
   this test reads the project's headers with) where the reference tree is present.
2. The adapter (HipVolumeRenderer.cpp) compiled with -DSMK_USE_REFERENCE_HEADERS against the
   reference's real MetaVolume.h / TLUT.h / gluvvPrimitive.h / gluvv.h, the build INTEGRATION.md
   prescribes: oracle/Makefile makes oracle/_ref/HipVolumeRenderer_refhdr.o where the reference tree
   is present; this test reads its symbols.

Both are built products of oracle/_ref/ (never in git, carried along with a built tree); the tests skip
where oracle/_ref/ was not built, as tests/test_perlin_ref.py does.
"""
import json
import os
import subprocess

import pytest

from header_decls import parse_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "simian-spacemonkey_amd", "host")
REF_DECLS = os.path.join(ROOT, "oracle", "_ref", "reference_decls.json")
REFHDR_OBJ = os.path.join(ROOT, "oracle", "_ref", "HipVolumeRenderer_refhdr.o")
# what VolumeRenderable needs from VolumeRenderer (VolumeRenderer.h:86-123), GLdouble spelled double
VOLUME_RENDERER_INNER = ["createVolume(int,Volume*)", "createVolume(int,Volume*,int)", "createTLUT()", "getColorMap()",
                         "renderVolume(float,double[16])", "renderVolume(float,double[16],float[2],float[2],float[2])",
                         "renderSlice(float[4][3],float)", "useBBox(int)", "useBBoxBrackets(int)"]


def _reference_decls():
    if not os.path.exists(REF_DECLS):
        pytest.skip("oracle/_ref not built (reference tree absent)")
    with open(REF_DECLS) as f:
        return json.load(f)


def _reference():
    classes, enums = {}, {}
    for h, d in _reference_decls().items():
        if h != "VolumeRenderer.h":
            classes.update(d["classes"])
            enums.update(d["enums"])
    return classes, enums


def test_every_compat_declaration_exists_in_the_reference_with_the_same_signature():
    cc, ce = parse_header(os.path.join(HOST, "gluvv_compat.h"))
    rc, re_ = _reference()
    assert {"Volume", "MetaVolume", "TLUT", "gluvvPrimitive", "gluvvGlobal", "gluvvVolRen", "gluvvPert"} <= set(cc)
    problems = []
    for cls, members in cc.items():
        if cls not in rc:
            problems.append("class %s does not exist in the reference" % cls)
            continue
        for key, decl in members.items():
            if key not in rc[cls]:
                problems.append("%s::%s is not a member of the reference's %s" % (cls, key, cls))
            elif rc[cls][key] != decl:
                problems.append("%s::%s is '%s' here, '%s' in the reference" % (cls, key, decl, rc[cls][key]))
    for name, vals in ce.items():
        if name not in re_:
            problems.append("enum %s does not exist in the reference" % name)
        elif re_[name] != vals:
            problems.append("enum %s: %s here, %s in the reference" % (name, vals, re_[name]))
    assert not problems, "\n".join(problems)
    # the two signatures the round-1 adapter got wrong stay pinned
    assert rc["TLUT"]["scaleAlpha(float)"] == "void" and cc["TLUT"]["scaleAlpha(float)"] == "void"
    assert "~gluvvPrimitive()" in rc["gluvvPrimitive"] and rc["gluvvPrimitive"]["~gluvvPrimitive()"] == ""  # not virtual


def test_adapter_compiles_against_the_reference_headers():
    if not os.path.exists(REFHDR_OBJ):
        pytest.skip("oracle/_ref not built (reference tree absent)")
    obj = REFHDR_OBJ
    # what it leaves for the reference's own objects to provide: gluvvPrimitive's defaults and TLUT's ctor/dtor
    syms = subprocess.run(["nm", "-C", "--undefined-only", str(obj)], capture_output=True, text=True).stdout
    assert "TLUT::TLUT(int)" in syms and "gluvvPrimitive::" in syms
    assert "TLUT::scaleAlpha" not in syms and "loadTransferTableRGBA" not in syms.replace("HipVolumeRenderer::loadTransferTableRGBA", "")


def test_hip_volume_renderer_has_the_inner_interface_of_volume_renderer():
    """what VolumeRenderable needs from VolumeRenderer (VolumeRenderer.h:86-123).  Every public method of the
    reference class that is not GL/NRRD plumbing must exist in HipVolumeRenderer with the same return type and parameter
    types (GLdouble is double, GL/gl.h)."""
    ref = _reference_decls()["VolumeRenderer.h"]["classes"]["VolumeRenderer"]
    ref = {k.replace("GLdouble", "double"): v for k, v in ref.items()}
    hc, _ = parse_header(os.path.join(HOST, "HipVolumeRenderer.h"))
    mine = hc["HipVolumeRenderer"]
    problems = []
    for key in VOLUME_RENDERER_INNER:
        if key not in ref:
            problems.append("the reference's VolumeRenderer has no %s (the test's list is stale)" % key)
        elif key not in mine:
            problems.append("HipVolumeRenderer lacks %s" % key)
        elif mine[key] != ref[key]:
            problems.append("%s returns '%s' here, '%s' in the reference" % (key, mine[key], ref[key]))
    assert not problems, "\n".join(problems)
