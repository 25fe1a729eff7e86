"""child process of tests/test_gpu_conv_route.py: the plain RPN head forward (conv_route None) on exact-grid cases under the environment the
parent set before the library read its knobs (SNN_SPARSE=0, or SNN_CONV_ROUTE=auto).  Prints one JSON line: per case the launch the conv
reported, route_stat and a digest of outputs and hidden planes."""
import json
import sys

import torch


def main(mode, cases):
    from tests import _conv_route as R
    from tests import _exact_grid as G
    dev = torch.device("cuda:0")
    out = {}
    for name, C, T, precision in cases:
        case = G.rpn_full_nibble_case() if name == "full_nibble" else G.rpn_t_case(C, T, "narrow" if precision == "bf16" else "wide")
        m = R.head_for(case, dev, precision)
        r = R.forward(m, [f.to(dev) for f in case["feats"]], None)
        out[name] = dict(path=r["path"], stat=r["stat"], digest=R.digest(r), mode=mode)
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1], json.loads(sys.argv[2]))
