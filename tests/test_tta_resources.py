"""CPU: the kernels of test-time augmentation must not spill.  hipcc cross-compiles their translation units for gfx950
with -Rpass-analysis=kernel-resource-usage (the parsing of tests/test_kernel_resources.py): ScratchSize 0 for every one of
them, and at least 2 waves per SIMD for the noisy per-sample forwards -- conv3x3_kernel<2, 1, TAIL 4 | 5, ..>, which hold a
whole pass's noise in registers on top of what the clean cube-fed forward holds and still count on two four-wave
workgroups per CU (or one eight-wave workgroup)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
NOISY = ("conv3x3_kernelILi2ELi1ELi4E", "conv3x3_kernelILi2ELi1ELi5E")      # MODE 2, MTW 1, TAIL 4 (range) / 5 (list)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_tta_kernels_have_no_scratch_and_the_noisy_forwards_keep_two_waves(tmp_path):
    files = ("conv3x3.hip", "ensemble.hip", "tta.hip")
    procs = [subprocess.Popen([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "-c",
                               os.path.join(ROOT, "cmlpl_amd", "csrc", f), "-o", str(tmp_path / (f + ".o")),
                               "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              text=True) for f in files]
    stderr = ""
    for pr in procs:
        _, err = pr.communicate(timeout=900)
        assert pr.returncode == 0, err[-2000:]
        stderr += err
    seen = {}
    for b in re.split(r"remark: Function Name: ", stderr)[1:]:
        name = b.split()[0]
        kind = next((k for k in NOISY + ("ensemble_views_kernel", "tta_patches_kernel", "tta_spectra_kernel") if k in name), None)
        if kind is None:
            continue
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1))
        print(name, "scratch", scratch, "waves/SIMD", occ)
        assert scratch == 0, (name, scratch)
        if kind in NOISY:
            assert occ >= 2, (name, occ)
        seen[kind] = seen.get(kind, 0) + 1
    # range and list, each as the four-wave and the eight-tile kernel; one views kernel per group width 1 .. 64
    assert seen == {NOISY[0]: 2, NOISY[1]: 2, "ensemble_views_kernel": 7, "tta_patches_kernel": 1, "tta_spectra_kernel": 1}, seen
