"""The ctypes signature table (h2o3_amd/ops/_abi.py) against the C prototypes
of the HIP sources, in both directions, and against the call sites.  Needs
neither a device nor a compiled library."""
import glob
import os
import re

from h2o3_amd.ops import _abi

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "h2o3_amd")
CSRC = os.path.join(ROOT, "ops", "csrc")

_PROTO = re.compile(r'^(extern "C" )?(int|void|long long) (h2o_\w+)\(([^()]*)\)\s*[{;]', re.M)
_ANY_DEF = re.compile(r'^[^\s/#}][^\n;=]*?\b(h2o_\w+)\(', re.M)
_BLOCK = re.compile(r'^extern "C" \{$', re.M)
_SCALARS = {"int": "i", "long long": "q", "unsigned long long": "Q", "float": "f", "double": "d"}
_RETURNS = {"int": "i", "long long": "q", "void": "v"}


def _kind(param):
    if "*" in param or param.split()[0] == "hipStream_t":
        return "P"
    words = [w for w in param.split() if w != "const"]
    return _SCALARS[" ".join(words[:-1])]       # KeyError: a type this parser does not know


def _close(text, i):
    """Offset of the brace that closes the block opened just before offset i."""
    depth = 1
    while depth:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
    return i


def parse(text):
    """{name: (return kind, argument kinds)} of the exported h2o_* functions of
    one HIP source.  A name declared and later defined must agree with itself."""
    text = re.sub(r"/\*.*?\*/", "", re.sub(r"//[^\n]*", "", text), flags=re.S)
    blocks = [(m.end(), _close(text, m.end())) for m in _BLOCK.finditer(text)]
    out = {}
    for m in _PROTO.finditer(text):
        assert m.group(1) or any(a <= m.start() < b for a, b in blocks), f"{m.group(3)}: not extern \"C\""
        params = [p.strip() for p in m.group(4).split(",") if p.strip()]
        sig = (_RETURNS[m.group(2)], "".join(_kind(p) for p in params))
        assert out.setdefault(m.group(3), sig) == sig, f"{m.group(3)}: declaration and definition differ"
    skipped = {m.group(1) for m in _ANY_DEF.finditer(text)} - set(out)
    assert not skipped, f"prototypes the parser skipped: {sorted(skipped)}"
    return out


def sources():
    return {os.path.splitext(os.path.basename(p))[0]: parse(open(p).read())
            for p in sorted(glob.glob(os.path.join(CSRC, "*.hip")))}


def mismatches(protos, table):
    """Differences between {lib: {name: (ret, args)}} of the sources and of the table."""
    bad = []
    for lib in sorted(set(protos) | set(table)):
        a, b = protos.get(lib, {}), table.get(lib, {})
        bad += [f"{lib}.{n}: only in the sources" for n in sorted(set(a) - set(b))]
        bad += [f"{lib}.{n}: only in the table" for n in sorted(set(b) - set(a))]
        bad += [f"{lib}.{n}: source {a[n]} != table {b[n]}" for n in sorted(set(a) & set(b)) if a[n] != b[n]]
    return bad


def test_every_source_yields_functions():
    src = sources()
    assert len(src) == len(glob.glob(os.path.join(CSRC, "*.hip"))) >= 12
    assert all(src.values()), [k for k, v in src.items() if not v]
    assert sum(len(v) for v in src.values()) == 95


def test_table_matches_prototypes():
    assert mismatches(sources(), _abi.signatures()) == []


def test_comparison_can_fail():
    src = sources()
    ret, args = src["tree_hist"]["h2o_hist_bm"]
    assert args[1] == "i"
    src["tree_hist"]["h2o_hist_bm"] = (ret, args[0] + "P" + args[2:])
    bad = mismatches(src, _abi.signatures())
    assert len(bad) == 1 and bad[0].startswith("tree_hist.h2o_hist_bm: source")
    one = parse('extern "C" int h2o_x(const float* a, long long n, hipStream_t s) { return 0; }')
    assert one == {"h2o_x": ("i", "PqP")}
    assert mismatches({"l": one}, {"l": {"h2o_x": ("i", "PiP")}}) != []


def test_called_names_are_known():
    """Every <lib>.h2o_x( call under h2o3_amd/ names a function of the table or
    an export of the host C++ libraries (native/*.cpp)."""
    known = {n for fns in _abi.signatures().values() for n in fns}
    for p in glob.glob(os.path.join(ROOT, "native", "*.cpp")):
        known |= set(re.findall(r"\b(h2o_\w+)\s*\(", open(p).read()))
    unknown = {}
    for p in glob.glob(os.path.join(ROOT, "**", "*.py"), recursive=True):
        for n in re.findall(r"\w\.(h2o_\w+)\(", open(p).read()):
            if n not in known:
                unknown.setdefault(n, os.path.relpath(p, ROOT))
    assert not unknown, unknown
