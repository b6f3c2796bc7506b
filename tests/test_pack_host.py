"""Host test of the weight packer: the stand-alone check (tools/pack_host_check.cpp over csrc/mdx_pack.cpp, the unit the library links)
built with the host compiler alone -- no HIP -- and run.  No GPU."""
from .util import run_host_check


def test_every_layout_decoded_by_the_host_check(tmp_path):
    """dense, stream, split dense and split stream packs, straight and transposed, of matrices that hit every padding branch, decoded
    through an inverse index map of the check's own and compared bit for bit; a centred view; the float16 range bookkeeping; the error
    string of a missing parameter"""
    run_host_check('pack_host_check', tmp_path, sources=('moldiff_amd/csrc/mdx_pack.cpp',))
