"""What keeps tests/test_gpu_stream_contract.py's case table complete, checked without a GPU: every entry of include/ewn_hip.h that takes
a stream has a case, the number of launch sites per source file is the one written down beside the site-to-case table, and the
environment overrides the library reads are the ones the header's conventions paragraph names."""
import glob
import os
import re

from tests import test_gpu_stream_contract as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ewn_gym_amd", "csrc")


def header():
    return open(os.path.join(ROOT, "include", "ewn_hip.h")).read()


def sources():
    return {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, "*"))) if os.path.isfile(p)}


def code(text):
    """the text without its comments: a `<<<` or a getenv in a comment is no site"""
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_every_stream_taking_entry_has_a_case():
    hdr = code(header())
    declared = set(re.findall(r"^(?:int|int64_t)\s+(ewn_\w+)\s*\([^;()]*\bvoid \*stream\)\s*;", hdr, re.M))
    assert len(declared) == 43 and "ewn_step" in declared and "ewn_puct_selfplay" in declared and "ewn_strerror" not in declared
    cased = set(entry for entry, _, _ in sc.CASES)
    assert declared == cased, declared ^ cased
    assert set(sc.STATEFUL) <= declared
    assert len(set(sc.IDS)) == len(sc.IDS) and set(sc.THREAD_SEQUENCE) <= set(sc.IDS)


def test_every_case_is_named_in_the_site_table():
    doc = sc.__doc__
    for entry in set(entry for entry, _, _ in sc.CASES):
        assert entry in doc, entry
    for cid, env in sc.CHILD_ENV.items():               # a case of a latched path: named with its override
        assert cid in doc and all(k in doc for k in env), cid
    assert sorted(sc.IN_PROCESS + list(sc.CHILD_ENV)) == sorted(sc.IDS)


def test_the_table_imports_without_torch():
    """the case table is plain data: with `import torch` failing, the module still imports and holds every case"""
    import subprocess
    import sys
    prog = ("import sys; sys.modules['torch'] = None\n"
            "from tests import test_gpu_stream_contract as m\n"
            "assert m.torch is None\n"
            "print(len(m.CASES), len(m.LAUNCH_SITES))")
    r = subprocess.run([sys.executable, "-c", prog], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == [str(len(sc.CASES)), str(len(sc.LAUNCH_SITES))]


def test_launch_site_counts():
    counts = {name: code(text).count("<<<") for name, text in sources().items()}
    counts = {k: v for k, v in counts.items() if v}
    assert counts == sc.LAUNCH_SITES, (counts, sc.LAUNCH_SITES)
    assert sum(counts.values()) == 49          # 47 kernels' sites and the two clears that were hipMemsetAsync
    memsets = {name: len(re.findall(r"\bhipMemset\w*\s*\(", code(text))) for name, text in sources().items()}
    assert {k: v for k, v in memsets.items() if v} == sc.MEMSET_SITES
    # every one of them is the asynchronous call and every launch names a stream: four launch parameters
    for name, text in sources().items():
        assert not re.findall(r"\bhipMemset\s*\(|\bhipMemcpy\s*\(|\bhip(?:Device|Stream)Synchronize\s*\(|\bhipMalloc\w*\s*\(|\bhipFree\w*\s*\(", code(text)), name
        for cfg in re.findall(r"<<<(.*?)>>>", code(text), re.S):
            depth, commas = 0, 0
            for ch in cfg:
                depth += ch == "("
                depth -= ch == ")"
                commas += ch == "," and depth == 0
            assert commas == 3, (name, cfg)


def test_environment_overrides_are_the_ones_the_header_names():
    read = set()
    for text in sources().values():
        read |= set(re.findall(r"\bgetenv\s*\(\s*\"(\w+)\"\s*\)", code(text)))
    hdr = header()
    para = hdr[hdr.index("No hidden global state"):hdr.index("Boards are int8")]
    named = set(re.findall(r"\bEWN_[A-Z0-9_]+\b", para))
    assert read == named, read ^ named
    assert len(read) == 6 and "six" in para
    latched = set()
    for text in sources().values():
        latched |= set(re.findall(r"static const \w+ \w+ = \[\]\s*\{[^}]*?getenv\s*\(\s*\"(\w+)\"", code(text)))
    assert latched == read - {"EWN_PUCT_TILE"}, latched
    assert para.index("EWN_PUCT_TILE") > para.index("latched") and "read at every" in para
