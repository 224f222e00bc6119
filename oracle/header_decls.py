"""Declarations of C++ headers as data: {class: {member key: normalised declaration}} and
{enum: [enumerators]}.  tests/test_compat_signatures.py compares the project's drop-in headers with the
reference's through it; oracle/Makefile runs it over the reference's headers where that tree is present:

    python3 header_decls.py <reference tree> _ref/reference_decls.json

(a build product under _ref/, never in git, like the other things built from the reference).
A member key is the name of a data member, or name(parameter types)[ const] of a member function.
"""
import json
import os
import re
import sys

# the reference headers the drop-in boundary touches
HEADERS = ("MetaVolume.h", "TLUT.h", "gluvv.h", "gluvvPrimitive.h", "VolumeRenderer.h")

KEYWORDS = {"unsigned", "signed", "int", "char", "float", "double", "long", "short", "void", "bool", "const"}


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#[^\n]*", " ", text, flags=re.M)
    return text


def _match_brace(text, i):
    depth = 0
    for j in range(i, len(text)):
        if text[j] == "{":
            depth += 1
        elif text[j] == "}":
            depth -= 1
            if depth == 0:
                return j
    raise ValueError("unbalanced braces")


def _flatten_body(body):
    """replace every nested {...} (inline function bodies) by ';'; nested enums are returned apart"""
    out, enums, i = [], {}, 0
    while i < len(body):
        if body[i] == "{":
            j = _match_brace(body, i)
            head = "".join(out)
            m = re.search(r"typedef\s+enum\s*$", head)
            if m:
                tail = re.match(r"\s*(\w+)\s*;", body[j + 1:])
                enums[tail.group(1)] = _enumerators(body[i + 1:j])
                out = [head[:m.start()]]
                i = j + 1 + tail.end()
                continue
            out.append(";")
            i = j + 1
        else:
            out.append(body[i])
            i += 1
    return "".join(out), enums


def _enumerators(body):
    return [re.sub(r"\s+", "", e) for e in body.split(",") if e.strip()]


def _norm_type(t):
    t = re.sub(r"\b(inline|static|explicit)\b", " ", t)
    t = re.sub(r"\s*([\*&])\s*", r"\1", t)
    return " ".join(t.split())


def _param_type(p):
    p = p.split("=")[0].strip()
    if not p:
        return ""
    arr = "".join(re.findall(r"\[[^\]]*\]", p))
    p = re.sub(r"\[[^\]]*\]", "", p)
    toks = re.findall(r"[\w:]+|[\*&]", p)
    words = [t for t in toks if t not in "*&"]
    if len(words) >= 2 and toks[-1] not in "*&" and toks[-1] not in KEYWORDS:
        toks = toks[:-1]  # the parameter's name
    return _norm_type(" ".join(toks)) + arr


def _members(body):
    """{name or signature: normalised declaration} of one class/struct body"""
    flat, enums = _flatten_body(body)
    flat = re.sub(r"\b(public|protected|private)\s*:", " ", flat)
    out = {}
    for st in flat.split(";"):
        st = " ".join(st.split())
        if not st:
            continue
        if "(" in st:
            m = re.match(r"^(?P<ret>.*?)(?P<name>~?\w+)\s*\((?P<params>.*)\)\s*(?P<const>const)?\s*(:.*)?$", st)
            assert m, st
            params = [p for p in (_param_type(p) for p in m.group("params").split(",")) if p and p != "void"]
            key = "%s(%s)%s" % (m.group("name"), ",".join(params), " const" if m.group("const") else "")
            out[key] = _norm_type(m.group("ret"))
        else:
            parts = [p.strip() for p in st.split(",")]
            m = re.match(r"^(?P<type>.*?)(?P<ptr>[\*&\s]*)(?P<name>\w+)(?P<arr>(\[\w*\])*)$", parts[0])
            assert m, st
            base = _norm_type(m.group("type"))
            for k, part in enumerate(parts):
                if k:
                    m = re.match(r"^(?P<ptr>[\*&\s]*)(?P<name>\w+)(?P<arr>(\[\w*\])*)$", part)
                    assert m, st
                out[m.group("name")] = base + m.group("ptr").replace(" ", "") + m.group("arr")
    return out, enums


def parse_header(path):
    text = _strip_comments(open(path, errors="replace").read())
    classes, enums = {}, {}
    for m in re.finditer(r"\b(class|struct)\s+(\w+)\s*(?::[^{;]*)?\{", text):
        end = _match_brace(text, m.end() - 1)
        members, nested = _members(text[m.end():end])
        classes[m.group(2)] = members
        for k, v in nested.items():
            enums["%s::%s" % (m.group(2), k)] = v
    for m in re.finditer(r"\btypedef\s+enum\s*\{", text):
        end = _match_brace(text, m.end() - 1)
        tail = re.match(r"\s*(\w+)\s*;", text[end + 1:])
        name = tail.group(1)
        if not any(name == k.split("::")[-1] for k in enums):
            enums[name] = _enumerators(text[m.end():end])
    return classes, enums


def main(ref_dir, out_path):
    out = {}
    for h in HEADERS:
        classes, enums = parse_header(os.path.join(ref_dir, h))
        out[h] = {"classes": classes, "enums": enums}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit("usage: header_decls.py <reference tree> <output .json>")
    main(sys.argv[1], sys.argv[2])
