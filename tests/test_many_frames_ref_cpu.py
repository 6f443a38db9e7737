"""Guard of the reference construction of tests/test_many_frames_gpu.py::test_training_gradient_at_100_frames: a direct fp64 oracle
gradient of 100 frames is out of reach (53 s for 20 frames), so that test builds its batch from two clips A, B and takes the
multiplicity-weighted mean of the two single-clip fp64 gradients as the batch gradient.  That holds because every detector loss is a
mean over clips and GroupNorm is per frame.  Here the fp64 oracle checks the identity itself on a small batch, [A, B, B] against
(g_A + 2 g_B) / 3: if an option ever makes a loss something other than a mean over clips, this fails before the GPU reference silently
goes wrong."""
import torch

from neural_marionette_amd.spec import DETECTOR_LOSS_KEYS
from test_train_detector_gpu import AIST, _setup, _oracle_grads_uncached


def test_batch_gradient_is_the_weighted_mean_of_clip_gradients():
    o, sd, vox = _setup(G=32, B=2, T=3, seed=11)
    A, B = vox[0:1], vox[1:2]
    batch = torch.cat([A, B, B]).contiguous()
    l_all, g_all, out_all = _oracle_grads_uncached(o, sd, batch, AIST, double=True)
    l_a, g_a, out_a = _oracle_grads_uncached(o, sd, A.contiguous(), AIST, double=True)
    l_b, g_b, out_b = _oracle_grads_uncached(o, sd, B.contiguous(), AIST, double=True)
    worst = 0.0
    for k in DETECTOR_LOSS_KEYS:
        va, vb, vall = (float(t[k].detach()) for t in (out_a, out_b, out_all))
        want = (va + 2.0 * vb) / 3.0
        e = abs(vall - want)
        worst = max(worst, e / max(1.0, abs(want)))
        assert e <= 1e-12 * max(1.0, abs(want)), (k, vall, want)
    assert abs(l_all - (l_a + 2.0 * l_b) / 3.0) <= 1e-12 * max(1.0, abs(l_all))
    num = den = 0.0
    for k, g in g_all.items():
        want = (g_a[k] + 2.0 * g_b[k]) / 3.0
        assert g.dtype == torch.float64
        num += ((g - want) ** 2).sum().item(); den += (want ** 2).sum().item()
    l2 = (num / den) ** 0.5
    print("fp64 oracle, [A, B, B] against (g_A + 2 g_B) / 3: worst loss term %.1e relative, whole-gradient relative L2 %.1e" % (worst, l2))
    assert den > 0.0 and l2 < 1e-12, l2
