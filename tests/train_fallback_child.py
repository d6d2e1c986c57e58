"""Child process of tests/test_gpu_train_edges.py::test_switched_kernels_in_a_fresh_child (not collected by pytest).

The HIP library and nn/autograd.py read their A/B switches once per process, so the kernels behind them (the vector-ALU
attention-backward and point-attention kernels, the three-launch BatchNorm, the unfused forks) only run in a process
started with the switches in its environment.  Usage: train_fallback_child.py valu|unfused; prints one JSON line
{"env": the switches as seen here, "errors": {case: {quantity: max error over the reference's scale}}}."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(mode):
    from tests.test_gpu_train_edges import CHILD_ENV, child_cases
    env = {k: os.environ.get(k) for k in CHILD_ENV[mode]}
    assert all(v is not None for v in env.values()), "started without the switches of mode %r: %r" % (mode, env)
    if mode == "unfused":
        from zeroshape_amd.nn import autograd as A
        assert not A.FUSE_FORKS
    errors = {name: run() for name, (run, _) in child_cases(mode).items()}
    print(json.dumps({"env": env, "errors": errors}, sort_keys=True))


if __name__ == "__main__":
    main(sys.argv[1])
