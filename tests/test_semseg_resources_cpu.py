"""The three segmenter kernels (csrc/semseg.hip) in the built libgimhip.so: gfx950 code objects (both 16-bit flavours), no scratch.
Read from the AMDGPU metadata notes like tests/test_kernel_resources_cpu.py; no GPU."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("_kernel_resources", os.path.join(ROOT, "tests", "test_kernel_resources_cpu.py"))
_kr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_kr)

KERNELS = ("ppm_pool_kernel<true>", "ppm_pool_kernel<false>", "ppm_upsample_concat_kernel<true>", "ppm_upsample_concat_kernel<false>",
           "seg_head_kernel(")


def test_semseg_kernels_target_gfx950_without_scratch():
    ks = _kr._kernels()          # asserts the gfx950 target of every code object it parses
    for key in KERNELS:
        hit = [(n, v) for n, v in ks.items() if key in n]
        assert hit, f"{key} not found in the library"
        for n, (regs, scratch, spills) in hit:
            assert scratch == 0 and spills == 0, f"{n}: {scratch} B scratch, {spills} spilled registers"
            assert regs <= 128, f"{n}: {regs} VGPRs"
