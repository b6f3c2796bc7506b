"""Host test of the weight packer: the stand-alone check (tools/pack_host_check.cpp over csrc/mdx_pack.cpp, the unit the library links)
built with the host compiler alone -- no HIP -- and run.  No GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_layout_decoded_by_the_host_check(tmp_path):
    """dense, stream, split dense and split stream packs, straight and transposed, of matrices that hit every padding branch, decoded
    through an inverse index map of the check's own and compared bit for bit; a centred view; the float16 range bookkeeping; the error
    string of a missing parameter"""
    cxx = os.environ.get('CXX') or shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'pack_host_check')
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', os.path.join(ROOT, 'tools', 'pack_host_check.cpp'),
                        os.path.join(ROOT, 'moldiff_amd', 'csrc', 'mdx_pack.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'pack_host_check ok' in r.stdout, r.stdout[-3000:]
