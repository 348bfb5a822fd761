"""One ``op_apply_result`` call of one named case on a complex64 tensor of ``2^--log2n`` (24) elements, for a counter
run of its own around it (profiles/op_apply_lds_counters.txt):

    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_ACTIVE_INST_LDS -d <dir> -- \\
        python tools/op_apply_pmc_case.py --case dense_2q_bits_3_7
    python tools/pmc_dump.py <dir> --match op_apply

The cases place one dense term so that its partners are read from LDS in different patterns: inside a 16-byte group
(bits 0, 1), in different groups (bits 3, 7), across the chunk boundary (bits 11, 12), six bits (D = 64)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from op_apply_timing import axes_of, hermitian, resident  # noqa: E402

CASES = {"dense_2q_bits_0_1": (0, 1), "dense_2q_bits_3_7": (3, 7), "dense_2q_bits_11_12": (11, 12),
         "d64_six_bits": (0, 3, 8, 12, 19, 23)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES), required=True)
    ap.add_argument("--log2n", type=int, default=24)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("op_apply_pmc_case.py runs on the GPU: none visible.")
    L = args.log2n
    gen = torch.Generator(device="cuda").manual_seed(L)
    xt = torch.view_as_complex(torch.randn((1 << L, 2), generator=gen, device="cuda", dtype=torch.float32))
    fn, ex = resident(xt)
    bits = CASES[args.case]
    terms = [(axes_of(L, bits), hermitian(np.random.default_rng(7), 1 << len(bits)))]
    buf = torch.empty((2,) * L, dtype=torch.complex64, device="cuda")
    ex.op_apply_result((2,) * L, terms, out_ptr=buf.data_ptr())
    torch.cuda.synchronize()
    print(args.case, ex.op_apply_variant((2,) * L, terms), float(buf.abs().max().item()))
    fn.close()


if __name__ == "__main__":
    main()
