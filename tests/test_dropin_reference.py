"""Drop-in check against the UNMODIFIED reference network code, recorded in tests/golden/reference_networks.json
(tests/golden/make_network_golden.py): ``networks/ccnet.py`` imports ``CrissCrossAttention`` from ``cc_attention`` (line 13)
and the ABN classes from ``inplace_abn``; with this repository on sys.path those names must resolve to the MI355X module
and this repository's restatement, the RCCA head must construct with it, and the parameter names / shapes must equal
those of the reference's own module so checkpoints interchange."""
import importlib
import json
import os

import pytest
import torch

from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def tables():
    with open(os.path.join(GOLDEN, "reference_networks.json")) as f:
        return json.load(f)


def shapes(table):
    return {k: tuple(v["shape"]) for k, v in table.items()}


def test_unmodified_ccnet_imports_our_module(tables):
    import ccnet_amd
    from ccnet_amd.segmodel import RCCAModule
    assert tables["ccnet_imports"]["cc_attention"] == ["CrissCrossAttention"]
    for mod, names in tables["ccnet_imports"].items():
        m = importlib.import_module(mod)
        assert os.path.dirname(os.path.dirname(os.path.abspath(m.__file__))) == ROOT, (mod, m.__file__)
        for name in names:
            assert hasattr(m, name), (mod, name)
    assert importlib.import_module("cc_attention").CrissCrossAttention is ccnet_amd.CrissCrossAttention
    head = RCCAModule(2048, 512, 19)                          # networks/ccnet.py:99-123, as ResNet builds it (:147)
    assert isinstance(head.cca, ccnet_amd.CrissCrossAttention)
    assert head.cca.query_conv.out_channels == 64 and head.cca.value_conv.out_channels == 512
    assert {k: tuple(v.shape) for k, v in head.state_dict().items()} == shapes(tables["RCCAModule(2048,512,19)"])


def test_state_dict_interchanges_with_reference_module(tables):
    from ccnet_amd.segmodel import RCCAModule
    ours = RCCAModule(2048, 512, 19).cca
    ref = tables["CrissCrossAttention(512)"]
    assert {k: tuple(v.shape) for k, v in ours.state_dict().items()} == shapes(ref)
    g = torch.Generator().manual_seed(0)
    sd_ref = {k: torch.randn(*v["shape"], generator=g).to(getattr(torch, v["dtype"])) for k, v in sorted(ref.items())}
    res = ours.load_state_dict(sd_ref, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in sd_ref.items():
        assert torch.equal(ours.state_dict()[k], v)
