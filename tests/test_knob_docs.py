"""The knobs paragraph of DESIGN.md (between <!-- knobs:begin --> and
<!-- knobs:end -->) against the sources, read as text, no GPU: every
environment variable the library reads is listed there, and every KMC_ name
listed there is read by the package (compile-time names carry a leading -D)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC, = glob.glob(os.path.join(ROOT, "*", "csrc"))
PKG_DIR = os.path.dirname(CSRC)


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _knobs_text():
    m = re.search(r"<!-- knobs:begin -->(.*?)<!-- knobs:end -->", _read(os.path.join(ROOT, "DESIGN.md")), re.S)
    assert m, "DESIGN.md has no knobs:begin / knobs:end markers"
    return m.group(1)


def _getenv_names():
    names = set()
    for path in glob.glob(os.path.join(CSRC, "*")):
        names.update(re.findall(r'getenv\(\s*"(KMC_[A-Z0-9_]+)"', _read(path)))
    return names


def _environ_names():
    names = set()
    for path in glob.glob(os.path.join(PKG_DIR, "*.py")):
        names.update(re.findall(r'os\.(?:environ(?:\.get\(|\[)|getenv\()\s*"(KMC_[A-Z0-9_]+)"', _read(path)))
    return names


def test_every_getenv_is_documented():
    read = _getenv_names()
    assert len(read) >= 20  # (the pattern still finds kmc_create's block)
    documented = set(re.findall(r"KMC_[A-Z0-9_]+", _knobs_text()))
    assert sorted(read - documented) == []


def test_every_documented_knob_is_read():
    listed = set(re.findall(r"(?<!-D)\bKMC_[A-Z0-9_]+", _knobs_text()))
    assert listed
    assert sorted(listed - _getenv_names() - _environ_names()) == []
