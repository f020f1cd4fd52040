"""Resources of the staged prepare kernels (blitzar_amd/csrc/msm/kernels.h,
k_prepare_addends_staged) from the compiler's own report, with the flags the library is built with.
The kernel's 40 KiB of LDS are a quarter of a compute unit's: the hash-only launch of a caller
table keeps four workgroups per compute unit only while the normalising path adds no static LDS, no
scratch and stays within the registers of four waves per SIMD."""
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
    src = "msm/msm_curve25519.hip"
    obj = tmp_path_factory.mktemp("resources") / "msm_curve25519.o"
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
    return {k: v for k, v in out.items() if "k_prepare_addends_staged" in k}


# (trait, Table) as they appear in the mangled name
STAGED = {"normalising_table": "17ed25519_niels_msmELb1E",
          "plain_table": "11ed25519_msmELb1E",
          "plain": "11ed25519_msmELb0E"}


@pytest.mark.parametrize("which", sorted(STAGED))
def test_staged_prepare_resources(usage, which):
    tag = STAGED[which]
    found = [v for k, v in usage.items() if tag in k]
    assert len(found) == 1, f"{which}: {sorted(usage)}"
    got = found[0]
    print(which, got)
    assert got["scratch"] == 0
    assert got["lds"] == 40960
    assert got["occupancy"] == 4
