"""INTEGRATION.md §6 lists the environment switches: every SSBA_* variable the library reads has a row there, and every row
names a variable that is still read (by the library, or by bench.py for rows marked `(bench.py)`)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ceres_slam_amd", "csrc")


def _library_reads():
    names = set()
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h", ".cpp")):
            names |= set(re.findall(r'getenv\(\s*"(SSBA_[A-Z0-9_]+)"', open(os.path.join(CSRC, f)).read()))
    return names


def _table_rows():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    i = text.index("\n## 6.")
    j = text.find("\n## ", i + 1)
    rows = {}
    for line in text[i:j if j >= 0 else len(text)].splitlines():
        m = re.match(r"\|\s*`(SSBA_[A-Z0-9_]+)[^`]*`([^|]*)\|", line)
        if m:
            rows[m.group(1)] = "(bench.py)" in m.group(2)
    return rows


def test_every_switch_the_library_reads_is_documented():
    reads, rows = _library_reads(), _table_rows()
    assert reads, "no getenv(\"SSBA_...\") found under ceres_slam_amd/csrc"
    missing = sorted(reads - set(rows))
    assert not missing, f"INTEGRATION.md §6 has no row for {missing}"


def test_every_documented_switch_is_read():
    reads, rows = _library_reads(), _table_rows()
    bench = open(os.path.join(ROOT, "bench.py")).read()
    stale = sorted(n for n, by_bench in rows.items() if not (f'"{n}"' in bench if by_bench else n in reads))
    assert not stale, f"INTEGRATION.md §6 documents switches nothing reads: {stale}"
