"""f0.F0Bank, the one holder of the f0 estimators behind VC and FeatureInputAMD, without a device: one table of names,
loaders that load once, refusals that name what they refuse and list the same methods everywhere, and FcpeLegacyAMD
as FcpeAMD with other checkpoint names."""
import numpy as np
import pytest
import torch

from rvc_amd import f0, f0mix, synthetic
from rvc_amd.extract import FeatureInputAMD
from rvc_amd.pipeline import VC, Config

PIPELINE_ARGS = ("", 0.0, 1, 3, 1, "v2", 0.33, 64, False, 1, ".pth", ".pt")


def holders(**kw):
    return VC(40000, Config("cpu"), **kw), FeatureInputAMD(device="cpu", **kw)


def test_one_table_of_names():
    for cls in (VC, FeatureInputAMD):
        assert issubclass(cls, f0.F0Bank)
        assert cls.CREPE_METHODS is f0.CREPE_METHODS and cls.HYBRID_EXTRA is f0.HYBRID_EXTRA
        assert cls.FCPE_LEGACY_PT == f0.F0Bank.FCPE_LEGACY_PT and cls.FCPE_LEGACY_PT.endswith("fcpe_legacy.pt")
    assert f0mix.CREPE_MEMBERS == tuple(f0.CREPE_METHODS) and set(f0mix.CREPE_MEMBERS) < set(f0mix.MEMBERS)
    assert "fcpe-legacy" in f0.METHODS and "fcpe-legacy" not in VC.HYBRID_EXTRA and "fcpe-legacy" not in f0mix.MEMBERS
    vc, fi = holders()
    for h in (vc, fi):  # every estimator is declared by the constructor
        assert h.rmvpe is h.fcpe is h.fcpe_legacy is h.pm is h.swipe is None and h.crepe == {}


def test_given_models_are_returned_without_file_access(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)  # no assets/ here: a loader that went to a file would fail
    given = dict(rmvpe=object(), crepe={"tiny": object()}, fcpe=object(), fcpe_legacy=object())
    for h in holders(**given):
        assert h._rmvpe() is given["rmvpe"] and h._crepe("tiny") is given["crepe"]["tiny"]
        assert h._fcpe() is given["fcpe"] and h._fcpe_legacy() is h._fcpe_legacy(required=False) is given["fcpe_legacy"]
        assert h.crepe is not given["crepe"]  # the holder's own dict: bench-style ``h.crepe[cap] = ...`` stays local
        h.pm, h.swipe = "pm", "swipe"
        assert h._pm() == "pm" and h._swipe() == "swipe" and h._swipe("cuda:1") == "swipe"


def test_loaders_load_once(tmp_path, monkeypatch):
    from rvc_amd import crepe, fcpe, fcpe_legacy, pm, rmvpe, swipe
    monkeypatch.chdir(tmp_path)
    (tmp_path / "assets" / "models" / "predictors").mkdir(parents=True)
    (tmp_path / VC.FCPE_LEGACY_PT).write_bytes(b"")
    calls = []

    def fake(kind):
        def load(*args):
            calls.append((kind,) + args)
            return [kind]
        return load

    for mod, cls, kind in ((rmvpe, "RMVPEAMD", "rmvpe"), (crepe, "CrepeAMD", "crepe"), (fcpe, "FcpeAMD", "fcpe"),
                           (fcpe_legacy, "FcpeLegacyAMD", "fcpe_legacy")):
        monkeypatch.setattr(getattr(mod, cls), "from_file", staticmethod(fake(kind)))
    monkeypatch.setattr(swipe, "SwipeAMD", fake("swipe"))
    monkeypatch.setattr(pm, "PitchPM", fake("pm"))
    for h in holders():
        del calls[:]
        for _ in range(3):
            got = [h._rmvpe(), h._crepe("tiny"), h._fcpe(), h._fcpe_legacy(), h._swipe(), h._pm()]
        assert [g[0] for g in got] == ["rmvpe", "crepe", "fcpe", "fcpe_legacy", "swipe", "pm"]
        assert got[0] is h.rmvpe and got[1] is h.crepe["tiny"] and got[4] is h.swipe and got[5] is h.pm
        assert sorted(c[0] for c in calls) == sorted(["rmvpe", "crepe", "fcpe", "fcpe_legacy", "swipe", "pm"])
        paths = {c[0]: c[1] for c in calls if c[0] not in ("swipe", "pm")}
        assert paths["fcpe_legacy"] == h.FCPE_LEGACY_PT and paths["crepe"].endswith("crepe_tiny.pth")
        assert all(p.startswith(f0.PREDICTORS) for p in paths.values())
        assert all(c[-1] == "cpu" for c in calls)  # each on the holder's device


def _refusal(call, name):
    with pytest.raises(NotImplementedError, match=name) as e:
        call()
    text = str(e.value)
    assert repr(name) in text
    return text.partition("; ")[2]  # the list of what the path has


def test_refusals_name_the_method_and_list_the_same_methods(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    vc, fi = holders()
    x = np.zeros(16000, np.float32)
    xt = torch.zeros(16000)  # a host tensor: every refusal comes before anything touches a device
    lists = [
        _refusal(lambda: vc.pipeline(None, None, 0, x, 0, "harvest", *PIPELINE_ARGS), "harvest"),
        _refusal(lambda: vc.f0_device(xt, 0, "dio"), "dio"),
        _refusal(lambda: fi.compute_f0(x, "yin"), "yin"),
        _refusal(lambda: vc.pipeline(None, None, 0, x, 0, "hybrid[rmvpe+pyin]", *PIPELINE_ARGS), "pyin"),
        _refusal(lambda: vc.f0_device(xt, 0, "hybrid[harvest+swipe]"), "harvest"),
        _refusal(lambda: fi.compute_f0(x, "hybrid[pm+crepe]"), "crepe"),
        _refusal(lambda: fi.compute_f0_hybrid("hybrid[fcpe+piptrack]", x), "piptrack"),
        _refusal(lambda: vc.f0_raw(xt, "harvest", 100), "harvest"),
        _refusal(lambda: f0mix.parse_hybrid("hybrid[rmvpe+fcpe]"), "fcpe"),  # f0mix alone holds no model
        _refusal(lambda: fi.compute_f0(x, "pm"), "pm"),  # extraction: pm only as a hybrid member
    ]
    assert len(set(lists)) == 1
    for method in ("rmvpe", "crepe-*", "pm", "swipe", "fcpe", "fcpe-legacy", "hybrid[...]"):
        assert method in lists[0]
    for h in (vc, fi):
        h.check_f0_method("hybrid[pm+swipe+fcpe+rmvpe+crepe-full]")
        with pytest.raises(NotImplementedError, match="fcpe-legacy.*fcpe_legacy=.*fcpe_legacy.pt"):
            h.check_f0_method("fcpe-legacy")
        with pytest.raises(NotImplementedError, match="fcpe-legacy.*fcpe_legacy=.*fcpe_legacy.pt"):
            h.check_f0_method("hybrid[swipe+fcpe-legacy]")
        h.fcpe_legacy = object()
        h.check_f0_method("fcpe-legacy")
        assert h.f0_members("hybrid[swipe + fcpe-legacy+swipe]") == ["swipe", "fcpe-legacy", "swipe"]
    for method in ("rmvpe", "pm", "swipe", "fcpe", "crepe-tiny", "crepe-full"):
        vc.check_f0_method(method)
    assert f0mix.parse_hybrid("hybrid[rmvpe+fcpe]", extra=("fcpe",)) == ["rmvpe", "fcpe"]
    with pytest.raises(NotImplementedError, match="9 members"):
        vc.check_f0_method("hybrid[" + "+".join(["swipe"] * 9) + "]")


class _Conv:
    """Stands in for ops.Conv, whose weight packing needs a device: keeps what it was built from."""

    def __init__(self, w, b, device=None):
        self.shape, self.bias, self.device = tuple(w.shape), tuple(b.shape), device


def test_fcpe_legacy_is_fcpe_under_other_names(monkeypatch):
    from rvc_amd import fcpe, fcpe_legacy
    monkeypatch.setattr(fcpe, "Conv", _Conv)
    monkeypatch.setattr(fcpe_legacy, "Conv", _Conv)
    base, legacy = fcpe.FcpeAMD, fcpe_legacy.FcpeLegacyAMD
    for name in ("__init__", "_latent", "f0_device", "_buffers", "_stem", "_conformer", "_conformer_weights", "_head",
                 "mel", "post", "latent", "from_file"):
        assert name not in vars(legacy) and getattr(legacy, name) is not None, name
    assert set(vars(legacy)) - {"__module__", "__doc__"} == {
        "NAME", "CONFIG", "CHANS", "STEM", "LAYER", "OUT", "THRESHOLD", "_check_config", "_layer_weights",
        "_extra_buffers", "performer", "self_attention", "_layer", "decode", "f0"}
    assert base.THRESHOLD == 0.006 and legacy.THRESHOLD == 0.03
    C = 8
    a = base(synthetic.fcpe_checkpoint(n_layers=2, hidden_dims=C), "cpu")
    b = legacy(synthetic.fcpe_legacy_checkpoint(n_layers=2, n_chans=C), "cpu")

    def entries(m):
        def shapes(v):
            if isinstance(v, _Conv):
                return ("conv", v.shape, v.bias, v.device)
            if torch.is_tensor(v):
                return (tuple(v.shape), v.dtype, str(v.device))
            return tuple(shapes(t) for t in v) if isinstance(v, tuple) else v
        top = {k: shapes(getattr(m, k)) for k in ("C", "n_layers", "basis", "conv0", "gn", "conv1", "norm", "proj",
                                                    "cent_table")}
        return top, [{k: shapes(L[k]) for k in ("ln", "up", "dw", "down")} for L in m.layers]

    assert entries(a) == entries(b)
    top, layers = entries(b)
    assert top["conv0"][1] == (C, 128, 3) and top["proj"][1] == (360, C, 1) and len(layers) == 2
    assert layers[0]["up"][1] == (4 * C, C, 1) and layers[0]["dw"][0][0] == (2 * C, 31)
    assert set(a.layers[0]) == {"ln", "up", "dw", "down"}
    assert set(b.layers[0]) == {"ln", "up", "dw", "down", "norm", "qkv", "to_out", "proj"}
    assert b.layers[0]["qkv"].shape == (3 * 512, C, 1) and b.layers[0]["to_out"].shape == (C, 512, 1)
    assert a._extra_buffers(7) == {} and b._extra_buffers(7) == {"qkv": (3 * 512, 7), "att": (512, 7)}
