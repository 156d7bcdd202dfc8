"""The training engines refuse a batch whose channel or class count is not the model's, on the host, before anything is copied or
launched (TrainEngineBase._prep: every train_step / eval_step / step_forward of every engine goes through it).  The first conv indexes X
by the model's channel count and the loss kernels index y and w by its class count: annotation files that decode to fewer mask channels
than the model has classes (loader.colored_to_categorical yields a channel per palette colour PRESENT beyond the first) were read past
their ends.  The counts are the MODEL's -- a resumed checkpoint's, not train_model's arguments -- and the loader does not matter."""
import warnings

import pytest
import torch

from interactive_unet import train_engine, train_engine_f32


def _engine(cls, dim, cin, ncls):
    """The host-side state _prep reads, without a GPU."""
    e = object.__new__(cls)
    e.dev, e.dim, e.cin, e.ncls = torch.device('cpu'), dim, cin, ncls
    return e


@pytest.mark.parametrize('cls', [train_engine.TrainEngine, train_engine.EncoderTrainEngine, train_engine.CoarseTrainEngine, train_engine_f32.TrainEngineF32])
def test_prep_refuses_other_channel_and_class_counts(cls):
    e = _engine(cls, 2, 1, 2)
    X, y = torch.zeros(2, 1, 8, 8, dtype=torch.float16), torch.zeros(2, 2, 8, 8, dtype=torch.float16)
    out = e._prep(X, y, y.clone())
    assert out[3:8] == (2, 1, 8, 8, 64) and out[8] == (64, 64, 64, 8, 1)
    assert e._prep(X, y, None)[2] is None
    for bx, by, bw, word in ((X, y[:, :1], y[:, :1], r'y \(2, 1, 8, 8\)'),                  # masks that decoded to one class
                             (X, y, y[:, :1], r'w \(2, 1, 8, 8\)'),
                             (X, torch.zeros(2, 3, 8, 8), None, '2 classes'),
                             (X.expand(2, 3, 8, 8), y, None, r'1 input channel\(s\)'),
                             (X, y[:, :, :4], None, 'grid'), (X, y[:1], None, 'grid'), (X[:, 0], y, None, 'the 2-D model')):
        with pytest.raises(ValueError, match=word):
            e._prep(bx, by, bw)
    e3 = _engine(cls, 3, 2, 3)
    X3, y3 = torch.zeros(1, 2, 4, 4, 8), torch.zeros(1, 3, 4, 4, 8)
    assert e3._prep(X3, y3, y3)[3:8] == (1, 4, 4, 8, 128)
    with pytest.raises(ValueError, match='the 3-D model'):
        e3._prep(X3[:, :, 0], y3[:, :, 0], None)
    with pytest.raises(ValueError, match='3 classes'):
        e3._prep(X3, y3[:, :2], y3[:, :2])


def test_the_counts_are_a_resumed_models_own(tmp_path):
    """A 3-class checkpoint resumed under train_model's default num_classes = 2: the engine takes its counts from the model, so 2-class
    batches are refused and 3-class ones pass."""
    from interactive_unet import unet
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        unet.UNet(num_channels=1, num_classes=3, pretrained=False).save_checkpoint(str(tmp_path / 'model.ckpt'))
        m = unet.UNet.load_from_checkpoint(checkpoint_path=str(tmp_path / 'model.ckpt'))
    assert (m.num_channels, m.num_classes) == (1, 3)
    for cls in (train_engine.TrainEngine, train_engine_f32.TrainEngineF32):
        src = __import__('inspect').getsource(cls.__init__)
        assert 'self.cin, self.ncls = model.num_channels, model.num_classes' in src      # where the real engines get them
    e = _engine(train_engine.TrainEngine, m.dim, m.num_channels, m.num_classes)
    X = torch.zeros(2, 1, 16, 16)
    with pytest.raises(ValueError, match='3 classes'):
        e._prep(X, torch.zeros(2, 2, 16, 16), torch.zeros(2, 2, 16, 16))
    e._prep(X, torch.zeros(2, 3, 16, 16), None)
