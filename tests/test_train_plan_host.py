"""Host test of the training operators' shared arithmetic: the stand-alone enumeration (tools/train_plan_host_check.cpp over
csrc/mdx_train_plan.h, the header csrc/mdx_train.hip and csrc/mdx_fast.cpp compile) of the split-partial layout, the weight-gradient
queue's plan, the LayerNorm backward's partial rows and the deferred reduction's record table.  No GPU."""
from .util import run_host_check


def test_train_plan_enumerated_by_the_host_check(tmp_path):
    """row ranges tile [0, M) in multiples of the row chunk; products, first-stage planes, bias partials and theirs are disjoint and end
    at the reported total; a chunked record's planes sit where the layout reserved them; blocks == gx * gy * S -- built from the real
    header with the host compiler, warnings as errors"""
    run_host_check('train_plan_host_check', tmp_path)
