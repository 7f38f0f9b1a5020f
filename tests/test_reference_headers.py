"""The C++ adapters' stand-in headers against the reference's own headers.  Nothing of the reference travels.

1. The IceTray build of the C++ adapters (clsim_amd/cxx/, -DCLSIMHIP_WITH_ICETRAY) is compiled with
   -I/root/reference/public FIRST on the include path: every <clsim/...> header the adapter and its glue include is the
   reference's own -- the abstract interfaces they derive from (public/clsim/I3CLSimStepToPhotonConverter.h:67-192,
   I3CLSimLightSourceToStepConverter.h:61-198), the 48- / 80-byte records, and the configuration classes whose private
   members the glue reads by name (private_access.h).  Stand-ins remain only for icetray/, dataclasses/, phys-services/,
   boost/ (tests/stubs/); tests/stubs/real_header_defs.cxx defines the members the real headers declare out of line.
   The binary then runs the same checks as tests/test_icetray_adapter.py.
2. Every stand-in under tests/stubs/clsim/ (used by the tests that do travel to the GPU box) is compared with the header it
   stands for: same virtual member functions in the same order (the vtable layout), with the same parameter lists, and
   the same set of constructors.  What these checks need of the reference headers is stored as SHA-256 hashes in
   tests/golden/reference_header_surfaces.json, so they run everywhere; where the reference tree is present they also check
   that file against it (regenerate: python -c "from tests.test_reference_headers import write_surfaces; write_surfaces()").
Part 1 needs the reference tree and is skipped where it is absent."""
import hashlib
import json
import os
import re
import subprocess

import pytest

from tests import common

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.path.join(ROOT, "clsim_amd", "cxx")
REF_PUBLIC = "/root/reference/public"
STUBS = os.path.join(ROOT, "tests", "stubs")

SURFACES = os.path.join(ROOT, "tests", "golden", "reference_header_surfaces.json")
HAVE_REFERENCE = os.path.isdir(os.path.join(REF_PUBLIC, "clsim"))


def build_against_reference_headers(tmp_path):
    exe = str(tmp_path / "icetray_adapter_real_headers")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-DI3CLSIM_WITHOUT_OPENCL", "-DCLSIMHIP_WITH_ICETRAY",
           "-I" + REF_PUBLIC, "-I" + STUBS, "-I" + CXX, "-H", "-o", exe, os.path.join(CXX, "icetray_adapter_test.cxx"),
           os.path.join(STUBS, "real_header_defs.cxx"), "-L" + os.path.join(ROOT, "clsim_amd"), "-lclsimhip",
           "-Wl,-rpath," + os.path.join(ROOT, "clsim_amd")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    included = set(re.findall(r"^\.+ (\S+)$", p.stderr, flags=re.M))
    return exe, included


@pytest.mark.skipif(not HAVE_REFERENCE, reason="the reference tree is not on this machine")
def test_adapters_compile_and_run_against_the_reference_headers(tmp_path):
    exe, included = build_against_reference_headers(tmp_path)
    clsim = sorted(h for h in included if "/clsim/" in h)
    assert clsim, "no clsim header was included?"
    # every clsim header came from the reference tree, none from the stand-ins
    assert all(h.startswith(REF_PUBLIC + "/clsim/") for h in clsim), [h for h in clsim if not h.startswith(REF_PUBLIC)]
    for must in ("I3CLSimStepToPhotonConverter.h", "I3CLSimLightSourceToStepConverter.h", "I3CLSimStep.h", "I3CLSimPhoton.h",
                 "I3CLSimMediumProperties.h", "function/I3CLSimFunctionRefIndexIceCube.h", "function/I3CLSimScalarFieldIceTiltZShift.h",
                 "random_value/I3CLSimRandomValueMixed.h", "random_value/I3CLSimRandomValueInterpolatedDistribution.h"):
        assert REF_PUBLIC + "/clsim/" + must in clsim, must
    out = subprocess.check_output([exe, "check", os.path.join(common.ICE, "spice_lea"), common.PHOTONICS["photonics_mie"]], text=True)
    assert out.count("medium round trip ok") == 3 and "icetray adapter ok" in out
    out = subprocess.check_output([exe, "lightsource_check", os.path.join(common.ICE, "spice_mie")], text=True)
    assert "light source adapter ok" in out


# ---- stand-in fidelity ----
def _strip(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    return text


def _macro_expand(text, stub_dir):
    """the stand-ins fold repeated virtuals into I3STUB_*_BOILERPLATE macros (function/I3CLSimFunction.h,
    random_value/I3CLSimRandomValue.h): expand them before comparing"""
    macros = {}
    for base in ("function/I3CLSimFunction.h", "random_value/I3CLSimRandomValue.h"):
        src = open(os.path.join(stub_dir, base)).read()
        for m in re.finditer(r"#define (I3STUB_\w+)\s*\\\n((?:.*\\\n)*.*)\n", src):
            macros[m.group(1)] = m.group(2).replace("\\\n", "\n")
    for name, body in macros.items():
        text = text.replace(name, body)
    return text


def _canon_params(params):
    """parameter types only: names, default values and spacing removed"""
    out = []
    depth = 0
    cur = ""
    for ch in params:
        if ch in "<(":
            depth += 1
        elif ch in ">)":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur)
            cur = ""
        else:
            cur += ch
    if cur.strip():
        out.append(cur)
    canon = []
    for p in out:
        p = p.split("=")[0].strip()
        p = re.sub(r"\bstd::size_t\b", "size_t", p)
        p = re.sub(r"\bboost::shared_ptr\b", "shared_ptr", p)
        m = re.match(r"^(.*?[\s&\*>])\s*([A-Za-z_]\w*)$", p)        # drop a trailing parameter name
        if m and m.group(2) not in ("double", "float", "int", "bool", "unsigned", "uint32_t", "uint64_t", "int32_t", "size_t", "I3Particle",
                                    "I3CLSimFlasherPulse", "AllParticles_t"):
            p = m.group(1)
        canon.append(re.sub(r"\s+", "", p))
    return tuple(canon)


def _balanced(s, start):
    """text between the parenthesis that opens just before `start` and its partner"""
    depth, i = 1, start
    while depth:
        depth += {"(": 1, ")": -1}.get(s[i], 0)
        i += 1
    return s[start:i - 1]


def class_surface(text, cls):
    """virtual member functions in declaration order and the constructor signatures of class `cls`"""
    m = re.search(r"\b(?:struct|class)\s+" + cls + r"\b([^;{]*)\{", text)
    assert m, cls
    base = re.search(r":\s*(?:public|private|protected)?\s*(I3CLSim\w+)", m.group(1))
    i = m.end()
    depth = 1
    while depth:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
    body = text[m.end():i - 1]
    flat = ""
    depth = 0
    for ch in body:                                   # drop inline function bodies and nested types
        if ch == "{":
            depth += 1
            if depth == 1:
                flat += ";"
        elif ch == "}":
            depth -= 1
        elif depth == 0:
            flat += ch
    virtuals, ctors = [], set()
    for decl in flat.split(";"):
        decl = " ".join(decl.split())
        decl = re.sub(r"^(public|private|protected)\s*:\s*", "", decl)
        if re.match(r"^virtual\s+~", decl):
            virtuals.append(("~", (), ""))
            continue
        mv = re.match(r"^virtual\s+(.*?)\b(\w+)\s*\((.*)\)\s*(const)?\s*(?:throw\s*\(\s*\))?\s*(?:=\s*0)?$", decl)
        if mv:
            virtuals.append((mv.group(2), _canon_params(mv.group(3)), mv.group(4) or ""))
            continue
        mc = re.match(r"^(?:explicit\s+)?" + cls + r"\s*\(", decl)
        if mc:
            ctors.add(_canon_params(_balanced(decl, mc.end())))
    return virtuals, ctors, (base.group(1) if base else None)


def stub_headers():
    out = []
    base = os.path.join(STUBS, "clsim")
    for d, _, files in os.walk(base):
        for f in sorted(files):
            if f.endswith(".h"):
                out.append(os.path.relpath(os.path.join(d, f), base))
    return sorted(out)


def reference_header_of(cls, rel):
    """the reference header that defines class `cls`: the stand-in's namesake, else wherever the class is defined"""
    first = os.path.join(REF_PUBLIC, "clsim", rel)
    cands = [first] + [os.path.join(d, f) for d, _, fs in os.walk(os.path.join(REF_PUBLIC, "clsim")) for f in sorted(fs) if f.endswith(".h")]
    for c in cands:
        if os.path.exists(c) and re.search(r"\b(?:struct|class)\s+" + cls + r"\b[^;{]*\{", _strip(open(c).read())):
            return c
    raise AssertionError("no reference header defines " + cls)


def _h(value):
    """what the fixture stores of a declaration: the SHA-256 of its canonical form"""
    return hashlib.sha256(repr(value).encode()).hexdigest()[:16]


def stub_classes(rel):
    stub = _strip(_macro_expand(open(os.path.join(STUBS, "clsim", rel)).read(), os.path.join(STUBS, "clsim")))
    classes = re.findall(r"\b(?:struct|class)\s+(I3CLSim\w+)\b[^;{]*\{", stub)
    assert classes, rel
    return stub, classes


def reference_surface(rel):
    """per class of stand-in `rel`, hashed: the reference class's base, its virtual members (in order and as a set), the names
    of its base's virtual members, the virtual members it adds to its base (in order) and its constructors"""
    out = {}
    for cls in stub_classes(rel)[1]:
        rv, rc, rbase = class_surface(_strip(open(reference_header_of(cls, rel)).read()), cls)
        base_names = {v[0] for v in class_surface(_strip(open(reference_header_of(rbase, rel)).read()), rbase)[0]} if rbase else set()
        out[cls] = {"base": _h(rbase), "virtuals": _h(rv), "virtual_set": sorted({_h(v) for v in rv}),
                    "base_virtual_names": sorted({_h(n) for n in base_names}),
                    "new_virtuals": _h([v for v in rv if v[0] not in base_names and v[0] != "~"]),
                    "ctors": sorted({_h(c) for c in rc})}
    return out


def write_surfaces():
    """needs the reference tree: writes tests/golden/reference_header_surfaces.json"""
    with open(SURFACES, "w") as f:
        json.dump({rel: reference_surface(rel) for rel in stub_headers()}, f, indent=1, sort_keys=True)
        f.write("\n")


@pytest.mark.parametrize("rel", stub_headers())
def test_stand_in_declares_what_the_reference_header_declares(rel):
    stub, classes = stub_classes(rel)
    with open(SURFACES) as f:
        stored = json.load(f)[rel]
    if HAVE_REFERENCE:
        assert reference_surface(rel) == stored, "the reference headers differ from %s: run write_surfaces()" % SURFACES
    for cls in classes:
        ref = stored[cls]
        sv, sc, sbase = class_surface(stub, cls)
        assert _h(sbase) == ref["base"], (cls, sbase)
        if sbase is None:
            # an interface root: same virtual functions in the same order (= the same vtable), same parameter types, same
            # constness; a virtual destructor only where the reference has one
            assert _h(sv) == ref["virtuals"], "%s: virtual members differ from the reference's\n stand-in: %s" % (cls, sv)
        else:
            # a derived class: overriders take their vtable slot from the base, so order is free; what the stand-in declares
            # virtual must exist in the reference class with the same signature, and virtuals the reference ADDS (new slots)
            # must all be there in the reference's order
            extra = [v for v in sv if _h(v) not in ref["virtual_set"] and v[0] != "~"]
            assert not extra, "%s: the stand-in declares virtuals the reference lacks: %s" % (cls, extra)
            new_stub = [v for v in sv if _h(v[0]) not in ref["base_virtual_names"] and v[0] != "~"]
            assert _h(new_stub) == ref["new_virtuals"], "%s: new virtual members differ from the reference's\n stand-in: %s" % (cls, new_stub)
        # every constructor the stand-in offers exists in the reference with the same parameter types
        missing = {c for c in sc if _h(c) not in ref["ctors"] and c != ()}
        assert not missing, "%s: the stand-in has constructors the reference lacks: %s" % (cls, missing)
