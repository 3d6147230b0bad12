"""The register-resident lane exchanges behind the canonical sums and the chains' integer scans (sf_device_math.hpp:
lane_swap over v_permlane32_swap / v_permlane16_swap, lane_xor_dpp, wave_scan_add / wave_scan_max / wave_sum / wave_max)
on the device, through the stand-alone program tools/ubench/canon_lanes.hip:

  * every lane distance exchanges with lane ^ off (lane numbers as payload, 32-bit and both words of a double);
  * block_sum_canon in the register form is bit-equal to a verbatim copy of the __shfl_xor form it replaces, for
    N = 1, 2, 3, 6, 11, 16 and 28, on 256 threads and on one wavefront -- random doubles over the whole exponent range,
    +-0, denormals and +-inf; a NaN total is compared by NaN-ness only -- and so is canon_reduce on 1, 2 and 4
    wavefronts at element counts that leave wavefronts of the canonical scheme empty, partly filled and looping;
  * the integer scans and reductions equal values computed on the host.

The program is built with the canonical-arithmetic flags of csrc/Makefile and run once, as a child process."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_lane_exchanges_sums_and_scans_on_the_device(tmp_path):
    exe = str(tmp_path / "canon_lanes")
    build = subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-vectorize", "-fno-slp-vectorize",
         os.path.join(ROOT, "tools", "ubench", "canon_lanes.hip"), "-o", exe],
        capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, (run.returncode, run.stdout[-4000:], run.stderr[-2000:])
    lines = run.stdout.splitlines()
    assert "directions: ok" in lines
    for n in (1, 2, 3, 6, 11, 16, 28):
        assert "sums N=%2d: ok" % n in lines
    assert "integers: ok" in lines
    assert lines[-1] == "canon_lanes: PASS"
    # the data must have exercised both kinds of comparison: NaN totals and ordinary ones
    words = [ln for ln in lines if ln.startswith("block_sum_canon reference totals:")]
    assert len(words) == 1
    n_words, n_nan = int(words[0].split()[3]), int(words[0].split()[5])
    assert 0 < n_nan < n_words // 2
