"""The BowVector CSR checks of the keyframe database (csrc/mcs_kfdb_guard.hip: mcs_kfdb_add, mcs_kfdb_detect_relocalisation, mcs_kfdb_detect_loop,
mcs_kfdb_score) on their own, without a GPU, through tests/cpp/kfdb_guard_driver.cpp.  Driver and guard translation unit are compiled by hipcc in host-only
mode, as tests/test_window_guards_cpu.py compiles its driver; the program makes no HIP call.  It is built with AddressSanitizer and UBSan on the host side
where that links (the bad-offset cases hand the checks a word array shorter than the offsets claim), and without them otherwise; no Python process runs
under a sanitizer.

The offsets are judged as a whole before any word is read: the library sizes and fetches the word array by offsets[n], so [0, 10, 4] must be refused
before row 0 is walked, and [0, -1] before anything is sized."""
import os
import re
import subprocess
import warnings

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multicol-slam_amd", "csrc")
OK, INVALID = 0, -1
FIRST = "offsets[0] must be 0"
MONOTONE = "offsets must be non-decreasing"
RANGE = "word id out of range"
ORDER = "word ids of a BowVector must be strictly ascending"
ADD = "mcs_kfdb_add: "

EXPECTED = {
    "ok": (OK, ""), "ok.nkf0": (OK, ""), "ok.empty_rows_between": (OK, ""), "ok.all_rows_empty": (OK, ""), "ok.one_word_vocabulary": (OK, ""),
    "offsets.first_above_0": (INVALID, FIRST),
    "offsets.decrease_after_large_row": (INVALID, ADD + MONOTONE),
    "offsets.negative_last": (INVALID, ADD + MONOTONE),
    "offsets.negative_last_after_rows": (INVALID, ADD + MONOTONE),
    "offsets.bare_text": (INVALID, MONOTONE),
    "word.equals_n_words": (INVALID, ADD + RANGE),
    "word.minus_1": (INVALID, ADD + RANGE),
    "word.equal_neighbours": (INVALID, ADD + ORDER),
    "word.descending_pair": (INVALID, ADD + ORDER),
    "word.descending_across_rows_is_fine": (OK, ""),
    "word.other_entry_point": (INVALID, "mcs_kfdb_score: " + ORDER),
    "first_above_0+decrease": (INVALID, FIRST),
    "decrease+bad_word_in_earlier_row": (INVALID, ADD + MONOTONE),
    "range+order_at_one_word": (INVALID, ADD + RANGE),
    "order_in_row_0+range_in_row_1": (INVALID, ADD + ORDER),
    "range_in_row_0+order_in_row_1": (INVALID, ADD + RANGE),
}


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _build(exe, extra):
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall",
           "-Wno-unused-function", "-I" + CSRC] + extra + ["-x", "hip", os.path.join(ROOT, "tests", "cpp", "kfdb_guard_driver.cpp"),
                                                          os.path.join(CSRC, "mcs_kfdb_guard.hip"), "-o", str(exe)]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    exe = tmp_path_factory.mktemp("kfdb_guards") / "kfdb_guard_driver"
    r = _build(exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    sanitized = r.returncode == 0
    if not sanitized:
        warnings.warn("the host sanitizers do not build here; the guard driver runs as a plain build:\n" + r.stdout.decode("utf-8", "replace")[-2000:])
        r = _build(exe, [])
        assert r.returncode == 0, r.stdout.decode("utf-8", "replace")
    p = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)   # the environment as it is
    if sanitized and p.returncode != 0 and b"ASan runtime does not come first" in p.stderr:
        # the sanitizer's runtime refuses to start in this environment (it found nothing: no case has run); the plain build runs the same cases
        warnings.warn("the sanitized guard driver does not start here; plain build instead:\n" + p.stderr.decode("utf-8", "replace")[-1000:])
        sanitized = False
        r = _build(exe, [])
        assert r.returncode == 0, r.stdout.decode("utf-8", "replace")
        p = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode("utf-8", "replace")[-4000:]
    out = {}
    for line in p.stdout.decode().splitlines():
        name, rc, text = line.split("\t")
        assert name not in out
        out[name] = (int(rc), text)
    out["__sanitized__"] = sanitized
    return out


def test_every_case_ran(results):
    print("built with host sanitizers:", results["__sanitized__"])
    assert sorted(k for k in results if k != "__sanitized__") == sorted(EXPECTED)


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_guard(results, name):
    print(name, results[name])
    assert results[name] == EXPECTED[name]


def test_every_text_is_covered():
    texts = {t for _, t in EXPECTED.values()}
    assert texts >= {FIRST, MONOTONE, ADD + MONOTONE, ADD + RANGE, ADD + ORDER}


def test_each_text_is_written_once():
    """the database's entry points keep no second copy of a check: over every file of csrc/, each text is a literal of the guard file alone, and mcs_kfdb.hip
    makes every BowVector CSR pass through it (its own texts are those of the connected-set offsets and of the device-side query check, which are other
    checks).  One exception, named here: mcs_capi_match.hip has an older "offsets[0] must be 0" of its own for the map points' descriptor rows, which is no
    BowVector CSR and not the database's."""
    src = {n: _read(n) for n in sorted(os.listdir(CSRC)) if n.endswith((".hip", ".h", ".inc"))}
    for text in (FIRST, MONOTONE, RANGE, ORDER):
        lit = '"%s"' % text
        counts = {n: s.count(lit) for n, s in src.items() if lit in s}
        want = {"mcs_kfdb_guard.hip": 1}
        if text == FIRST:
            want["mcs_capi_match.hip"] = 1
        assert counts == want, (text, counts)
    assert re.search(r"\bhip[A-Z]\w*\s*\(|HIPCHK|<<<", src["mcs_kfdb_guard.hip"]) is None, "the guard unit makes no HIP call"
    k = src["mcs_kfdb.hip"]
    add = k[k.index("int mcs_kfdb_add("):k.index("int mcs_kfdb_erase(")]
    assert add.index("guard_bow_offsets(") < add.index("off[nkf]") < add.index("fetch(w,") < add.index("guard_bow_words(")


def test_library_lists_the_guard_unit():
    mk = _read("Makefile")
    assert " mcs_kfdb_guard.hip " in mk
