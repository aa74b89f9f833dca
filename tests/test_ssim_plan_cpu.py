"""The host side of nsk_image_ssim without a GPU: host/test/ssim_plan_test runs csrc/nsk_ssim_plan.h (window, level sizes, the MS-SSIM
combine) alone under AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nice-slam-cpp_amd", "host")


def test_ssim_plan_test_under_the_sanitizers():
    subprocess.check_call(["make", "-s", "-C", HOST, "ssim_plan_test"])
    r = subprocess.run([os.path.join(HOST, "ssim_plan_test")], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "ssim_plan_test: ok" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
