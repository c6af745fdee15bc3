"""CPU: the host side of fused validation -- the two new C-ABI symbols, the save-path rules, get_current_visuals, image
writing through the torch path on a CPU model, and the C2M_VAL_FUSED switch.  The model tests follow the `Fake` pattern of
test_host_logic.py (validation logic only: no nets)."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_new_symbols_at_abi_6():
    import c2m_amd
    hdr = open(os.path.join(REPO, "include", "c2m_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(c2m_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(c2m_amd.LIB_PATH)
    for name in ("c2m_val_metrics_workspace_bytes", "c2m_val_metrics_f32"):
        assert name in declared and hasattr(lib, name), name
    assert lib.c2m_abi_version() == 6 and c2m_amd._lib.ABI_VERSION == 6
    # pure size arithmetic, no device: [B][tiles][3] float64, and 0 for a cropped window below 11 pixels
    L = c2m_amd.lib()
    th, tw = c2m_amd.ops.val_metrics_tile()
    assert (th, tw) == tuple(int(re.search(rf"#define C2M_VAL_TILE_{a}\s+(\d+)", hdr).group(1)) for a in "HW")
    assert L.c2m_val_metrics_workspace_bytes(2, th + 10 + 8, tw + 10 + 8, 4) == 2 * 1 * 3 * 8
    assert L.c2m_val_metrics_workspace_bytes(2, th + 11 + 8, 2 * tw + 10 + 8, 4) == 2 * 4 * 3 * 8
    assert L.c2m_val_metrics_workspace_bytes(1, 18, 40, 4) == 0 and L.c2m_val_metrics_workspace_bytes(1, 19, 19, 4) == 24


def test_cpu_tensors_are_rejected_by_the_new_ops():
    import c2m_amd
    from mmsr.utils import metrics
    x = torch.rand(1, 3, 24, 24)
    with pytest.raises(c2m_amd.C2MError):
        c2m_amd.ops.val_metrics(x, x)
    with pytest.raises(c2m_amd.C2MError):
        metrics.validation_metrics_fused(x, x)
    with pytest.raises(c2m_amd.C2MError):
        metrics.tensor2img_u8(x)


def _fake(opt):
    from mmsr.models.ref_restoration_model import RefRestorationModel

    class Fake(RefRestorationModel):   # validation logic only: no nets, SR = GT + a perturbation
        def __init__(self):
            self.opt = opt
            self.device = torch.device('cpu')
            self.rank = 0
            self.is_train = bool(opt.get('is_train'))

        def feed_data(self, data):
            self.gt = data['img_in']
            self.img_in_lq = data['img_in_lq']

        def test(self):
            self.output = (self.gt + 0.02 * torch.sin(40 * self.gt)).clamp(0, 1)
            return self.output
    return Fake()


def _items(n, with_paths=True, padded=False):
    g = torch.Generator().manual_seed(1)
    items = []
    for k in range(n):
        d = {'img_in': torch.rand(1, 3, 40, 44, generator=g), 'img_in_lq': torch.rand(1, 3, 10, 11, generator=g)}
        if with_paths:
            d['lq_path'] = [f'/data/val/img_{k:03d}.png']
        if padded:
            d['padding'], d['original_size'] = True, (36, 41)
        items.append(d)
    return items


class _Loader(list):
    class dataset:   # noqa: N801
        opt = {'name': 'CUFED5'}


def test_save_path_rules():
    train = _fake({'is_train': True, 'name': 'exp', 'suffix': 'x', 'path': {'visualization': '/v'}})
    assert train._save_img_path('img_000', 'CUFED5', 5000) == os.path.join('/v', 'img_000', 'img_000_5000.png')
    test = _fake({'is_train': False, 'name': 'exp', 'suffix': None, 'path': {'visualization': '/v'}})
    assert test._save_img_path('img_000', 'CUFED5', 0) == os.path.join('/v', 'CUFED5', 'img_000_exp.png')
    test.opt['suffix'] = 'x4'
    assert test._save_img_path('img_000', 'CUFED5', 0) == os.path.join('/v', 'CUFED5', 'img_000_exp_x4.png')
    with pytest.raises(ValueError, match='visualization'):
        _fake({'is_train': False, 'name': 'exp', 'path': {}})._save_img_path('a', 'b', 0)
    names = test._img_names
    assert names({'lq_path': ['/d/a.b/007_0.png']}, 3, 1) == ['007_0'] and names({'lq_path': '/d/008.jpg'}, 3, 1) == ['008']
    assert names({}, 3, 1) == ['3'] and names({}, 3, 2) == ['3_0', '3_1'] and names({'lq_path': ['/d/a.png']}, 4, 2) == ['a', '4_1']


def test_get_current_visuals_has_the_reference_keys():
    m = _fake({'scale': 4})
    item = _items(1)[0]
    m.feed_data(item)
    m.test()
    vis = m.get_current_visuals()
    assert list(vis) == ['img_in_lq', 'rlt', 'gt']
    assert torch.equal(vis['rlt'], m.output) and torch.equal(vis['gt'], item['img_in']) and torch.equal(vis['img_in_lq'], item['img_in_lq'])
    assert all(v.device.type == 'cpu' and not v.requires_grad for v in vis.values())
    del m.gt
    assert list(m.get_current_visuals()) == ['img_in_lq', 'rlt']


def test_cpu_model_saves_through_the_torch_path(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    import numpy as np
    from mmsr.utils import metrics
    opt = {'scale': 4, 'is_train': False, 'name': 'exp', 'suffix': 's', 'path': {'visualization': str(tmp_path)}}
    m = _fake(opt)
    items = _Loader(_items(2, padded=True) + _items(1, with_paths=False))
    plain = _fake(dict(opt)).nondist_validation(items, 0, None, False)
    assert not list(tmp_path.iterdir())
    res = m.nondist_validation(items, 0, None, True)
    assert res == plain and res['count'] == 3
    want = ['2_exp_s.png', 'img_000_exp_s.png', 'img_001_exp_s.png']
    assert sorted(os.listdir(tmp_path / 'CUFED5')) == want and os.listdir(tmp_path) == ['CUFED5']
    for k, f in ((0, 'img_000_exp_s.png'), (1, 'img_001_exp_s.png'), (2, '2_exp_s.png')):
        m.feed_data(items[k])
        sr = m.test()
        if 'padding' in items[k]:
            sr = sr[..., :36, :41]
        rgb = metrics.tensor2img_device(sr).flip(-1).to(torch.uint8)[0].numpy()
        got = np.asarray(Image.open(tmp_path / 'CUFED5' / f))
        assert got.shape == rgb.shape and np.array_equal(got, rgb), f


def test_fused_entry_gets_the_padded_tensors_and_the_valid_window(tmp_path, monkeypatch):
    """A stub in place of the op: the model hands over the whole (padded) tensors with valid_hw, asks for the RGB image only
    when it saves, and writes what the op returned."""
    Image = pytest.importorskip("PIL.Image")
    import numpy as np
    from mmsr.utils import metrics
    calls = []

    def stub(sr, gt, crop_border=4, valid_hw=None, images=None):
        calls.append((tuple(sr.shape), tuple(gt.shape), crop_border, valid_hw, images))
        vh, vw = valid_hw or sr.shape[-2:]
        out = metrics.validation_metrics(sr[..., :vh, :vw], gt[..., :vh, :vw], crop_border=crop_border)
        if images:
            out['sr_u8'] = torch.full((sr.shape[0], vh, vw, 3), 7 + len(calls), dtype=torch.uint8)
        return out
    monkeypatch.setattr(metrics, 'validation_metrics_fused', stub)
    opt = {'scale': 4, 'crop_border': 2, 'is_train': True, 'name': 'exp', 'path': {'visualization': str(tmp_path)}}
    m = _fake(opt)
    m._fused_validation = lambda sr, gt: True
    items = _items(1, padded=True) + _items(2)[1:]
    res = m.nondist_validation(items, 77, None, True)
    assert calls == [((1, 3, 40, 44), (1, 3, 40, 44), 2, (36, 41), 'rgb'), ((1, 3, 40, 44), (1, 3, 40, 44), 2, None, 'rgb')]
    got = np.asarray(Image.open(tmp_path / 'img_000' / 'img_000_77.png'))
    assert got.shape == (36, 41, 3) and (got == 8).all()
    got = np.asarray(Image.open(tmp_path / 'img_001' / 'img_001_77.png'))
    assert got.shape == (40, 44, 3) and (got == 9).all()
    del calls[:]
    again = m.nondist_validation(items, 78, None, False)
    assert [c[4] for c in calls] == [None, None] and again == res
    assert sorted(os.listdir(tmp_path / 'img_000')) == ['img_000_77.png']
    torch_path = _fake(opt)
    assert torch_path.nondist_validation(items, 78, None, False) == res       # and the CPU decision is the composition
    assert len(calls) == 2 and torch_path._fused_validation(torch.zeros(1), torch.zeros(1)) is False


def test_true_scalar_division_leaves_cpu_results_alone():
    from mmsr.utils import metrics
    g = torch.Generator().manual_seed(2)
    a, b = torch.rand(2, 3, 30, 33, generator=g), torch.rand(2, 3, 30, 33, generator=g)
    plain = metrics.validation_metrics(a, b)
    with metrics.true_scalar_division():
        inside = metrics.validation_metrics(a, b)
        assert torch.equal(a / 255.0, a.div(255.0)) and (a / 2).dtype == torch.float32
        assert torch.equal(torch.div(torch.arange(7), 2, rounding_mode='floor'), torch.arange(7) // 2)
    assert all(torch.equal(plain[k], inside[k]) for k in plain)


def test_switch_parsing():
    code = ("import importlib, json, os, sys\n"
            "sys.path.insert(0, sys.argv[1])\n"
            "os.environ.pop('C2M_VAL_FUSED', None)\n"
            "import mmsr.models.ref_restoration_model as m\n"
            "out = {'unset': m._VAL_FUSED}\n"
            "for v in ('1', '0', ''):\n"
            "    os.environ['C2M_VAL_FUSED'] = v\n"
            "    out[v] = importlib.reload(m)._VAL_FUSED\n"
            "print('RESULT ' + json.dumps(out))\n")
    run = subprocess.run([sys.executable, "-c", code, os.path.join(REPO, "c2-matching_amd")], capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    got = json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert got == {'unset': True, '1': True, '0': False, '': True}
    readme = open(os.path.join(REPO, "README.md")).read()
    assert re.search(r"\| `C2M_VAL_FUSED` \| `1` \|", readme)
