"""Resources of k_accumulate<ed25519_niels_msm> (blitzar_amd/csrc/msm/kernels.h,
accumulate_lds_gather) from the compiler's own report, with the flags the library is built with.
The loop runs at three waves per SIMD: at most 168 VGPRs and no scratch.  Its LDS is one 7168-byte
region per wavefront (msm/lds_gather.h), 28672 bytes per workgroup of four: three workgroups per
compute unit take 84 KB of the 160 and leave room for a k_reduce workgroup beside them."""
import os
import re
import shutil
import subprocess

import pytest


def _hipcc():
    from blitzar_amd import build
    return build.HIPCC if os.path.exists(build.HIPCC) else shutil.which("hipcc")


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if _hipcc() is None:
        pytest.skip("hipcc is not installed")
    from blitzar_amd import build
    src = "msm/msm_curve25519_niels_accumulate.hip"
    obj = tmp_path_factory.mktemp("resources") / "niels_accumulate.o"
    r = subprocess.run([_hipcc(), *build.FLAGS, *build.TU_FLAGS.get(src, []), "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(build.CSRC, src), "-o", str(obj)],
                       capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-4000:]
    fields = {"scratch": r"ScratchSize \[bytes/lane\]: (\d+)", "lds": r"LDS Size \[bytes/block\]: (\d+)",
              "occupancy": r"Occupancy \[waves/SIMD\]: (\d+)", "vgprs": r" VGPRs: (\d+)"}
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        for key, pattern in fields.items():
            m = re.search(pattern, line)
            if m and name is not None:
                out[name][key] = int(m.group(1))
    return {k: v for k, v in out.items() if "k_accumulate" in k}


def test_niels_accumulate_resources(usage):
    found = [v for k, v in usage.items() if "17ed25519_niels_msm" in k]
    assert len(found) == 1, sorted(usage)
    got = found[0]
    print(got)
    assert got["scratch"] == 0
    assert got["vgprs"] <= 168
    assert got["lds"] == 4 * 7168
    assert got["occupancy"] == 3
