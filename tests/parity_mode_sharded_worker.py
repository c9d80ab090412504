"""Worker of tests/test_gpu_parity_mode.py: the parity mode on a row-sharded model.  One rank (gloo, world size 1) whose collective hooks stay
installed (GBRL_HIP_FORCE_COLLECTIVE=1, set by the parent), so the engine takes the row-sharded code path on ONE GPU.  argv: port case_name out_npz"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))


def _refused(fn):
    try:
        fn()
    except RuntimeError as e:
        return str(e)
    return ""


def main():
    port, name, out = sys.argv[1], sys.argv[2], sys.argv[3]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = port
    import torch
    import torch.distributed as dist
    import gbrl_amd
    from gbrl_amd.dist import install_torch_collective
    import cases as K
    from helpers import load_golden
    dist.init_process_group("gloo", rank=0, world_size=1)
    case, g, (X, Xc, G, y) = load_golden(name)
    dev = torch.device("cuda:0")
    keep = []
    # "reference" after the hooks
    a = gbrl_amd.GBRL(**K.ctor_kwargs(case))
    keep.append(install_torch_collective(a, dev))
    set_after_install = _refused(lambda: a.set_parity_mode("reference"))
    mode_after_refusal = a.get_parity_mode()
    # the hooks after "reference"
    b = gbrl_amd.GBRL(parity_mode="reference", **K.ctor_kwargs(case))
    install_after_set = _refused(lambda: keep.append(install_torch_collective(b, dev)))
    # "exact_argmax" and "default" are accepted, and the step runs
    res = {}
    for mode in ("exact_argmax", "default"):
        m = gbrl_amd.GBRL(**K.ctor_kwargs(case))
        coll = install_torch_collective(m, dev)
        keep.append(coll)
        m.set_parity_mode(mode)
        pred = np.asarray(K.drive(m, case, X, Xc, G, y))
        res.update({mode + "/" + k: np.asarray(v) for k, v in m.get_ensemble_data().items() if k in K.ENSEMBLE_KEYS})
        res[mode + "/pred"] = pred
        res[mode + "/calls"] = coll.calls
        res[mode + "/mode"] = m.get_parity_mode()[0]
    np.savez(out, set_after_install=set_after_install, install_after_set=install_after_set, mode_after_refusal=mode_after_refusal[0], **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
