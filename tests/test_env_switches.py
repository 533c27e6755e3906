"""The EEGCLIP_* environment switches the code reads are exactly the ones DESIGN.md's "Environment switches" subsection documents (no GPU, no kernel)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "eeg_image_decode_amd")
NAME = re.compile(r"EEGCLIP_[A-Z0-9_]+")
READ = re.compile(r"os\.environ|getenv\(|setdefault")


def switches_read_by_the_code():
    files = glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True)
    files += [f for ext in ("hip", "h") for f in glob.glob(os.path.join(PKG, "csrc", "*." + ext))]
    found = {}
    for path in files:
        with open(path, encoding="utf-8") as f:
            for line in f:
                if READ.search(line):
                    for name in NAME.findall(line):
                        found.setdefault(name, os.path.relpath(path, ROOT))
    return found


def switches_documented():
    with open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8") as f:
        text = f.read()
    m = re.search(r"^### Environment switches.*?\n(.*?)(?=^#{1,6} )", text, re.M | re.S)
    assert m, "DESIGN.md has no 'Environment switches' subsection"
    return set(NAME.findall(m.group(1)))


def test_design_md_lists_exactly_the_switches_the_code_reads():
    read, documented = switches_read_by_the_code(), switches_documented()
    assert len(read) >= 10                                   # (the scan found the package: EEGCLIP_GEMM_PRECISION, EEGCLIP_STEP_PLAN, ...)
    undocumented = {n: read[n] for n in set(read) - documented}
    assert not undocumented, f"read by the code, missing from DESIGN.md: {undocumented}"
    stale = documented - set(read)
    assert not stale, f"named in DESIGN.md, read by nothing: {sorted(stale)}"
