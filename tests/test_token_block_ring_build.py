"""The token-block kernels (csrc/token_block.hip) as the compiler builds them for gfx950: no register spills in any of the six block kernels, the
forward's weight loads really are the pinned inline-asm ring (not a silent fall-back to the compiler's schedule), the counted waits hold in the
generated code (tools/check_asm_ring.py) -- and that tool counts STORES as vmcnt operations, since the fragments carried across a phase boundary
are waited for with stores in between."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = [f"token_block_{k}_kernelILb{t}E" for k in ("fwd", "bwd_a", "bwd_b") for t in (1, 0)]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("tb_ring") / "token_block.s"
    csrc = os.path.join(ROOT, "eeg_image_decode_amd", "csrc")
    from eeg_image_decode_amd import build                            # the library's own compiler flags: the check is about THAT code generation
    subprocess.run([HIPCC, *build.FLAGS, "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only", "-o", str(out), os.path.join(csrc, "token_block.hip")],
                   check=True, cwd=csrc, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return str(out), out.read_text()


def _metadata(text, kernel):
    """the amdhsa.kernels metadata entry of `kernel` as {key: value}"""
    blocks = [b for b in text.split("  - .agpr_count:")[1:] if re.search(r"\.name:\s+\S*" + re.escape(kernel), b)]
    assert len(blocks) == 1, kernel
    return dict(re.findall(r"^\s+\.(\w+):\s+(\S+)\s*$", blocks[0], flags=re.M))


def _body(text, kernel):
    m = re.search(r"^(_ZN\S*" + re.escape(kernel) + r"\S*):.*?^\s*s_endpgm", text, flags=re.M | re.S)
    assert m, kernel
    return m.group(0)


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_block_kernel_spills_a_register(asm, kernel):
    """(as built: forward 252 / 254 VGPRs train / eval, backward part A 234 / 222, part B 153 / 156; the test prints each kernel's figures)"""
    md = _metadata(asm[1], kernel)
    print(kernel, {k: md[k] for k in ("vgpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count", "private_segment_fixed_size")})
    assert int(md["vgpr_spill_count"]) == 0
    assert int(md["sgpr_spill_count"]) == 0
    assert int(md["private_segment_fixed_size"]) == 0


@pytest.mark.parametrize("kernel", KERNELS[:2])
def test_the_forward_ships_the_pinned_ring(asm, kernel):
    """S1, q | k | v (both head pairs), S4 and S7 run on the ring; S6 is recorded as kept on the compiler's schedule (CHANGELOG).  A lower bound of the
    inline-asm loads that must then be in the kernel: a GEMM whose first two k-steps are handed in issues 6 k-steps x NT tiles x (hi, lo) itself, S1 all 8;
    the q | k | v pass exists once per tile-orientation mask (tb_qkv_variant: 7, 3, 0 -- the compiler may merge the two waves' variants that share mask 7)
    and per head-pair round.  Requests for the next GEMM come on top."""
    body = _body(asm[1], kernel)
    n = len(re.findall(r";;#ASMSTART\s*\n\s*global_load_dwordx4", body))
    print(kernel, "inline-asm ring loads:", n)
    s1 = 8 * 2 * 2
    s4_s7 = 2 * 6 * 2 * 2
    qkv = 3 * 2 * 6 * 3 * 2
    assert n >= s1 + s4_s7 + qkv


def test_the_counted_waits_hold_in_the_generated_code(asm):
    import check_asm_ring
    assert check_asm_ring.check(asm[0]) == 0


STORES = """
_Z4kernv:
	;;#ASMSTART
	global_load_dwordx4 v[4:7], v[2:3], off
	;;#ASMEND
	global_store_dwordx4 v[2:3], v[20:23], off
	global_store_dwordx2 v[2:3], v[24:25], off offset:16
	global_store_dword v[2:3], v26, off offset:32
	;;#ASMSTART
	s_waitcnt vmcnt(3)
	;;#ASMEND
	v_mfma_f32_16x16x32_bf16 v[12:15], v[4:7], v[16:19], v[12:15]
	s_endpgm
"""


def test_the_checker_counts_a_store_as_a_vmcnt_operation(tmp_path):
    """a load, then N = 3 unconditional stores, then vmcnt(N) and a use: the load has landed (in-order retirement).  vmcnt(N + 1) may leave it
    outstanding and is reported -- and so is vmcnt(N) when one of the stores sits behind a branch that may skip it (a conditional store counts
    as zero)."""
    import check_asm_ring

    def run(text):
        f = tmp_path / "k.s"
        f.write_text(text)
        return check_asm_ring.check(str(f))

    assert run(STORES) == 0
    assert run(STORES.replace("s_waitcnt vmcnt(3)", "s_waitcnt vmcnt(4)")) == 1
    conditional = STORES.replace("\tglobal_store_dword v[2:3], v26, off offset:32\n",
                                 "\ts_cbranch_execz .LBB0_2\n\tglobal_store_dword v[2:3], v26, off offset:32\n.LBB0_2:\n")
    assert run(conditional) == 1
    assert run(conditional.replace("s_waitcnt vmcnt(3)", "s_waitcnt vmcnt(2)")) == 0
