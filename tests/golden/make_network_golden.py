#!/usr/bin/env python3
"""Generate the network-level fixtures from an UNMODIFIED checkout of the upstream CCNet source tree.

    python tests/golden/make_network_golden.py <path to the upstream CCNet checkout>

Writes, for tests/test_dropin_reference.py and tests/test_segmodel.py (which then need nothing outside this repository):

``reference_networks.json``
    the names ``networks/ccnet.py`` imports from the two packages this repository replaces (``cc_attention``,
    ``inplace_abn``), and the state_dict tables (key -> shape, dtype) of the upstream ``CrissCrossAttention(512)``,
    ``RCCAModule(2048, 512, 19)`` and ``Seg_Model(19, recurrence=2)``.  The upstream ``inplace_abn`` is a compiled package,
    so the network is built on this repository's restatement of it (its state_dict keys are those of the real package).
``seg_model_65x65.npz``
    the upstream network's own forward (eval mode, its pure-python criss-cross attention) and its ``CriterionDSN`` on a
    65x65 input.  The weights are this repository's ``Seg_Model(19, recurrence=2)`` built under ``torch.manual_seed(0)``
    with the attention's gamma set to 0.6 and seeded running statistics; the test rebuilds them the same way and checks
    a fingerprint of the state_dict before it compares.
"""
import ast
import importlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REPLACED = ("cc_attention", "inplace_abn")


def table(module):
    return {k: {"shape": list(v.shape), "dtype": str(v.dtype).replace("torch.", "")} for k, v in module.state_dict().items()}


def cpu_inf(B, H, W):
    # the values of the upstream INF (cc_attention/functions.py:11-12) without its hard-coded .cuda()
    return -torch.diag(torch.tensor(float("inf")).repeat(H), 0).unsqueeze(0).repeat(B * W, 1, 1)


def seeded_weights():
    """This repository's Seg_Model under manual_seed(0), gamma 0.6, seeded running statistics (what the test rebuilds)."""
    from ccnet_amd.segmodel import Seg_Model
    torch.manual_seed(0)
    m = Seg_Model(19, recurrence=2)
    with torch.no_grad():
        for mod in m.modules():
            if type(mod).__name__ == "CrissCrossAttention":
                mod.gamma.fill_(0.6)
        for mod in m.modules():
            if hasattr(mod, "running_var"):
                mod.running_mean.normal_(0, 0.1), mod.running_var.uniform_(0.8, 1.2)
    return m.state_dict()


def fingerprint(state):
    return np.array([sum(float(v.double().sum()) for v in state.values()),
                     sum(float(v.double().abs().sum()) for v in state.values())])


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "networks")):
        sys.exit(__doc__)
    ref = os.path.abspath(sys.argv[1])
    sys.path[:0] = [ref, ROOT]               # upstream cc_attention / networks / loss; this repository's inplace_abn
    sys.path.insert(2, os.path.join(ROOT, "tests"))
    state = seeded_weights()                  # (imports ccnet_amd before the upstream cc_attention is imported: no clash)
    networks = importlib.import_module("networks.ccnet")
    functions = importlib.import_module("cc_attention.functions")
    criterion = importlib.import_module("loss.criterion")
    assert functions.__file__.startswith(ref) and importlib.import_module("inplace_abn").__file__.startswith(ROOT)

    imports = {}
    with open(os.path.join(ref, "networks", "ccnet.py")) as f:
        for node in ast.walk(ast.parse(f.read())):
            if isinstance(node, ast.ImportFrom) and node.module and node.module.split(".")[0] in REPLACED:
                imports.setdefault(node.module, []).extend(a.name for a in node.names)

    theirs = networks.Seg_Model(19, recurrence=2)
    tables = {
        "ccnet_imports": imports,
        "CrissCrossAttention(512)": table(functions.CrissCrossAttention(512)),
        "RCCAModule(2048,512,19)": table(networks.RCCAModule(2048, 512, 19)),
        "Seg_Model(19,recurrence=2)": table(theirs),
        "Seg_Model(19,recurrence=2).parameters": sum(p.numel() for p in theirs.parameters()),
    }
    path = os.path.join(HERE, "reference_networks.json")
    with open(path, "w") as f:
        json.dump(tables, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {path} ({os.path.getsize(path) / 1e3:.0f} kB)")

    theirs.load_state_dict(state, strict=True)
    theirs.eval()
    for mod in theirs.modules():
        if type(mod).__name__ == "CrissCrossAttention":
            mod.INF = cpu_inf
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, 3, 65, 65, generator=g)
    labels = torch.randint(0, 19, (1, 65, 65), generator=g)
    labels[0, :5] = 255
    with torch.no_grad():
        out, aux = theirs(x)
        loss = criterion.CriterionDSN()([out, aux], labels)
    path = os.path.join(HERE, "seg_model_65x65.npz")
    np.savez(path, x=x.numpy(), labels=labels.numpy(), out=out.numpy(), aux=aux.numpy(), loss=np.array([float(loss)]),
             fingerprint=fingerprint(state))
    print(f"wrote {path} ({os.path.getsize(path) / 1e3:.0f} kB); logits {tuple(out.shape)}, loss {float(loss):.6f}")


if __name__ == "__main__":
    main()
