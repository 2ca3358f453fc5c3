"""The library's source list (no GPU, no compile): the #include graph of the three translation
units of csrc/ and of the two behaviour-cloning units stays inside rl_rocket_amd.build.sources() (what source_hash() and up_to_date() read), no file
of csrc/ is an orphan, no .hip file includes another, and tools/ab_exact_cap.py's anchors still
match the exact solver's text."""
import importlib.util
import os
import re

import pytest

from rl_rocket_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rl_rocket_amd", "csrc")
SEARCH = [CSRC, os.path.join(ROOT, "include")]  # the -I directories of build.command()
INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', re.M)


def includes(path):
    """The quoted includes of `path` that resolve next to it or in the build's -I directories."""
    with open(path) as f:
        names = INCLUDE.findall(f.read())
    found = []
    for name in names:
        for d in [os.path.dirname(path)] + SEARCH:
            p = os.path.normpath(os.path.join(d, name))
            if os.path.isfile(p):
                found.append(p)
                break
    return found


@pytest.fixture(scope="module")
def reached():
    # the three units of csrc/ and the two behaviour-cloning units, whose shared kernel text lies in csrc/
    seen, todo = set(), [B.SRC, B.SRC_EXACT, B.SRC_COLLECT, B.SRC_BC, B.SRC_BC_DISCRETE]
    while todo:
        p = os.path.normpath(todo.pop())
        if p not in seen:
            seen.add(p)
            todo += includes(p)
    return seen


def test_every_included_file_is_a_source(reached):
    assert len(reached) > 3  # the roots include something: the scan works
    assert reached <= set(B.sources())


def test_no_orphan_in_csrc(reached):
    files = {os.path.join(CSRC, f) for f in os.listdir(CSRC) if os.path.isfile(os.path.join(CSRC, f))}
    assert files - reached == set()


def test_sources_sorted_and_used_by_hash_and_freshness(monkeypatch, tmp_path):
    src = B.sources()
    assert src == sorted(src) and B.HEADER in src
    assert {B.SRC, B.SRC_EXACT, B.SRC_COLLECT} <= set(src)
    # source_hash() and up_to_date() read the list: a file added to it changes both
    extra = tmp_path / "extra.inc"
    extra.write_text("// new\n")
    out = tmp_path / "lib.so"
    out.write_text("")
    newest = max(os.path.getmtime(p) for p in src + [B.__file__])
    os.utime(out, (newest + 10, newest + 10))
    os.utime(extra, (newest + 20, newest + 20))
    monkeypatch.setattr(B, "OUT", str(out))
    h0 = B.source_hash()
    assert B.up_to_date()
    monkeypatch.setattr(B, "sources", lambda: src + [str(extra)])
    assert B.source_hash() != h0
    assert not B.up_to_date()


def test_no_hip_file_includes_a_hip_file(reached):
    for p in reached:
        if p.endswith(".hip"):
            assert [q for q in includes(p) if q.endswith(".hip")] == [], p


def test_ab_exact_cap_anchors_match_once():
    spec = importlib.util.spec_from_file_location("ab_exact_cap", os.path.join(ROOT, "tools", "ab_exact_cap.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(tool.INC) as f:
        text = f.read()
    assert os.path.normpath(tool.INC) == os.path.join(CSRC, "rocket_dopri5.inc")
    assert len(tool.PATCH) == 3
    for anchor, _ in tool.PATCH:
        assert text.count(anchor) == 1, anchor
