"""Host test of the training operators' shared arithmetic: the stand-alone enumeration (tools/train_plan_host_check.cpp over
csrc/mdx_train_plan.h, the header csrc/mdx_train.hip and csrc/mdx_fast.cpp compile) of the split-partial layout, the weight-gradient
queue's plan, the LayerNorm backward's partial rows and the deferred reduction's record table.  No GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_train_plan_enumerated_by_the_host_check(tmp_path):
    """row ranges tile [0, M) in multiples of the row chunk; products, first-stage planes, bias partials and theirs are disjoint and end
    at the reported total; a chunked record's planes sit where the layout reserved them; blocks == gx * gy * S -- built from the real
    header with the host compiler, warnings as errors"""
    cxx = os.environ.get('CXX') or shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'train_plan_host_check')
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', os.path.join(ROOT, 'tools', 'train_plan_host_check.cpp'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'train_plan_host_check ok' in r.stdout, r.stdout[-3000:]
