"""One-off behaviour check for changes to the training operators' host arithmetic (csrc/mdx_train_plan.h; development tool): prints what
the four C entry points mdx_op_wgrad_layout, mdx_op_wgrad_plan, mdx_op_ln_relu_bwd_rows and mdx_op_ln_relu_bwd_ws return over the grid
of tools/train_plan_host_check.cpp, one line per call, so that the library of a tree before and of a tree after such a change can be
compared with `diff`.  ctypes only.  No GPU.

  python tools/train_plan_dump.py LIB > OUT.txt        LIB: path of a libmoldiff_hip.so (default: this tree's)
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS = (0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 6279, 154666, 600000)
NKS = (1, 4, 6, 16, 32, 54, 64, 128, 256)
FS = (1, 32, 54, 64, 128, 256, 1024)


def main(path):
    L = ctypes.CDLL(path)
    i64, i32, p64 = ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(ctypes.c_int64)
    L.mdx_op_wgrad_layout.argtypes = [i64, i64, i64, i32, i32, p64, p64]
    L.mdx_op_wgrad_plan.argtypes = [i64, i64, i64, i32, i32, i64, i64, i32, p64]
    L.mdx_op_ln_relu_bwd_rows.argtypes, L.mdx_op_ln_relu_bwd_rows.restype = [i64], i64
    L.mdx_op_ln_relu_bwd_ws.argtypes, L.mdx_op_ln_relu_bwd_ws.restype = [i64, i32], ctypes.c_size_t
    out = sys.stdout
    for M in MS:
        out.write(f'ln_rows M={M}: {L.mdx_op_ln_relu_bwd_rows(M)}\n')
        for F in FS:
            out.write(f'ln_ws M={M} F={F}: {L.mdx_op_ln_relu_bwd_ws(M, F)}\n')
        for N in NKS:
            for K in NKS:
                for splits in (1, 2, 7, (M + 2047) // 2048):
                    for half in (0, 1):
                        S, b = i64(), i64()
                        rc = L.mdx_op_wgrad_layout(M, N, K, splits, half, ctypes.byref(S), ctypes.byref(b))
                        out.write(f'layout M={M} N={N} K={K} splits={splits} half={half}: rc={rc} S={S.value} bias_off={b.value}\n')
                    for dt in range(4):
                        for aligned in (0, 1):
                            o = (i64 * 8)()
                            rc = L.mdx_op_wgrad_plan(M, N, K, splits, dt, N, K, aligned, o)
                            out.write(f'plan M={M} N={N} K={K} splits={splits} dt={dt} aligned={aligned}: rc={rc} {" ".join(map(str, o))}\n')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'moldiff_amd', 'libmoldiff_hip.so'))
