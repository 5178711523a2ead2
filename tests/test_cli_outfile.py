"""OutFile (kmertools_amd/csrc/host/outfile.hpp), the one writer of every output file of the command line, through the
hidden `kmertools debug-outfile <dir>`: a directory that does not exist, /dev/full with 10 bytes (the failure shows at
close) and with 1 MiB (at the write; the same message), writes after a failure, a scope left without close(), 9 MiB in
pieces that straddle the flush threshold read back, a second close().  Under the plain build and the asan / tsan builds
of tests/test_oracle_sanitize.py.  No GPU."""
import pathlib
import subprocess

import pytest

from test_oracle_sanitize import CSRC, BIN, SAN_ENV, _clean


@pytest.fixture(scope="module")
def cli_builds():
    subprocess.check_call(["make", "-C", str(CSRC), "asan", "tsan"], stdout=subprocess.DEVNULL)
    return {"plain": BIN / "kmertools", "asan": BIN / "kmertools_asan", "tsan": BIN / "kmertools_tsan"}


@pytest.mark.parametrize("which", ["plain", "asan", "tsan"])
def test_outfile_paths(cli_builds, tmp_path, which):
    assert pathlib.Path("/dev/full").exists()
    r = subprocess.run([str(cli_builds[which]), "debug-outfile", str(tmp_path)], capture_output=True, env=SAN_ENV, timeout=600)
    _clean(r.stderr)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-2000:]
    assert r.stderr == b"", r.stderr[-2000:]
    assert r.stdout == b"outfile ok\n"
    assert list(tmp_path.iterdir()) == []        # it removes what it wrote
