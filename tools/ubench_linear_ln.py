"""Fused Linear + LayerNorm launch against the two launches, per shape (development tool; GPU box).  MDX_LIB = alternative build."""
import torch

import evalbench as EB
EB.use_lib_from_env()
from moldiff_amd import train_ops as T  # noqa: E402


def us(fn):
    return EB.timed(fn, 30)[0] * 1e3


def main():
    dev = torch.device('cuda:0')
    M = 154666
    print(f'{"K":>4s} {"N":>4s} {"fused us":>9s} {"linear us":>10s} {"ln us":>7s}')
    for K, N in ((64, 256), (256, 256), (128, 128), (64, 32), (64, 64), (256, 64)):
        x = torch.randn(M, K, device=dev).half()
        w = torch.randn(N, K, device=dev) * K ** -0.5
        b, g, be = torch.randn(N, device=dev), torch.rand(N, device=dev) + 0.5, torch.randn(N, device=dev)
        with torch.no_grad(), T.precision('fp16'):
            tf = us(lambda: T.linear_ln_relu(x, w, b, g, be))
            pre = T.linear(x, w, b)
            tl = us(lambda: T.linear(x, w, b))
            tn = us(lambda: T.ln_relu(pre, g, be, True))
        print(f'{K:4d} {N:4d} {tf:9.1f} {tl:10.1f} {tn:7.1f}', flush=True)


if __name__ == '__main__':
    main()
