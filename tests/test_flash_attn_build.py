"""The flash kernels with transposed scores (csrc/self_attn.hip at head dims 64 and 80, csrc/vae_attn.hip) as the compiler builds them for gfx950: none of the
18 instantiations spills a register or uses scratch, and each keeps the number of waves per SIMD it had before the head-dim-80 kernel was folded into
self_attn's template and the K / V staging into csrc/flash16.h (read from the kernel metadata of that build; a wave's registers, VGPRs + AGPRs, are
`.vgpr_count`, and 512 of them per SIMD lane give 5 waves up to 96, 4 up to 128, 3 up to 168, 2 up to 256)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
LIMIT = {5: 96, 4: 128, 3: 168, 2: 256}                                # most registers per wave at that many waves per SIMD
# (source file, kernel name as the Itanium ABI mangles its template arguments, waves per SIMD)
KERNELS = [("self_attn", f"self_attn_kernelILb{f}ELi{qt}ELb{c}ELi64EE", 2 if qt == 2 else 4) for qt in (2, 1) for c in (0, 1) for f in (1, 0)]
KERNELS += [("self_attn", f"self_attn_kernelILb{f}ELi1ELb0ELi80EE", 3) for f in (1, 0)]
KERNELS += [("vae_attn", f"vae_attn_kernelILb{f}ELi{nc}EE", {1: 5, 2: 3, 3: 2, 4: 2}[nc]) for nc in (1, 2, 3, 4) for f in (1, 0)]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("flash_attn")
    csrc = os.path.join(ROOT, "eeg_image_decode_amd", "csrc")
    from eeg_image_decode_amd import build                            # the library's own compiler flags: the check is about THAT code generation
    text = {}
    for f in ("self_attn", "vae_attn"):
        subprocess.run([HIPCC, *build.FLAGS, "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only", "-o", str(out / (f + ".s")),
                        os.path.join(csrc, f + ".hip")], check=True, cwd=csrc, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text[f] = (out / (f + ".s")).read_text()
    return text


def _metadata(text, kernel):
    """the amdhsa.kernels metadata entry of `kernel` as {key: value}"""
    blocks = [b for b in text.split("  - .agpr_count:")[1:] if re.search(r"\.name:\s+\S*" + re.escape(kernel), b)]
    assert len(blocks) == 1, kernel
    return dict(re.findall(r"^\s+\.(\w+):\s+(\S+)\s*$", blocks[0], flags=re.M), agpr_count=blocks[0].split()[0])


def test_these_are_all_the_kernels_of_the_family(asm):
    assert len(KERNELS) == 18
    assert sum(t.count("  - .agpr_count:") for t in asm.values()) == 18


@pytest.mark.parametrize("src,kernel,waves", KERNELS, ids=[k for _, k, _ in KERNELS])
def test_no_spill_and_the_occupancy_is_kept(asm, src, kernel, waves):
    md = _metadata(asm[src], kernel)
    print(kernel, {k: md[k] for k in ("vgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count", "private_segment_fixed_size")},
          f"-> {waves} waves per SIMD (<= {LIMIT[waves]})")
    assert int(md["vgpr_spill_count"]) == 0
    assert int(md["sgpr_spill_count"]) == 0
    assert int(md["private_segment_fixed_size"]) == 0
    assert int(md["vgpr_count"]) <= LIMIT[waves]
