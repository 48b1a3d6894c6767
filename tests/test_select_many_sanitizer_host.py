"""The host side of the six population-selection calls over ssc_select_many_item -- the walks over n_items caller structs,
every rejection the header lists and the tables that return SSC_OK without a launch -- under AddressSanitizer +
UndefinedBehaviorSanitizer: tests/sanitizer/select_many_args.c, a stand-alone program, linked against the sanitized host build
of libssc that tests/sanitizer/build.py makes.  No GPU: every call fails validation or has nothing to launch."""
import importlib.util
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                reason="hipcc not available")
HERE = os.path.dirname(os.path.abspath(__file__))


def test_item_walks_under_asan_ubsan():
    spec = importlib.util.spec_from_file_location("ssc_sanitizer_build", os.path.join(HERE, "sanitizer", "build.py"))
    sb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sb)
    sb.build()                                   # the sanitized libssc_asan.so (cached under tests/_build/asan/)
    src, exe = os.path.join(HERE, "sanitizer", "select_many_args.c"), os.path.join(sb.OUT, "select_many_args")
    subprocess.check_call([sb.HIPCC, "-O1", "-g", "-x", "c", src, "-I" + os.path.join(sb.ROOT, "include"), "-o", exe,
                           "-L" + sb.OUT, "-lssc_asan", "-Wl,-rpath," + sb.OUT] + sb.SAN)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "all expectations hold" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
