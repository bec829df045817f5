"""FeatureExtractor: image paths or arrays in, descriptors out -- the reference's torchreid/utils/feature_extractor.py
(:13-152) for the three-modality model.  The input of a tracker or a retrieval service is detector crops, every one of its
own size: each modality's chunk is resized, scaled and normalised by ONE ragged device call (DeviceTransform.ragged), and
the chunks all have `batch_size` rows, so the executor keeps one workspace however many images arrive."""
import numpy as np
import torch

from .data.transforms import IMAGENET_MEAN, IMAGENET_STD, DeviceTransform

_said_unpretrained = False


class FeatureExtractor(object):
    """callable([RGB, NI, TI]) -> descriptors [B, 2304] on the device.  Each member of the triple is one of
        - a list of strings (image paths)
        - a list of numpy.ndarray, each uint8 of shape (H, W, 3); every image may have its own size
        - a single string (image path)
        - a single numpy.ndarray of shape (H, W, 3)
        - a float torch.Tensor of shape (B, 3, H, W) or (3, H, W): already preprocessed, it reaches the model as it is
          (cut into the same chunks as everything else)
    and all three hold the same number of images.

    Args (the reference's, then three of this implementation):
        model_name (str): model name.
        model_path (str): path to model weights (load_pretrained_weights; ignored when empty or not a file).
        image_size (sequence): image height and width.
        pixel_mean, pixel_std (list): normalisation; pixel_norm=False: mean 0, std 1.
        device (str): 'cuda' (or a specific GPU); there is no CPU execution path.
        verbose (bool): print the model name and its parameter count.
        model: an already built model, used as it is instead of building one (model_name / model_path are then unused).
        batch_size (int): rows per forward; the last chunk is padded with copies of its last row, which are dropped again.
        compute_dtype: passed to build_model (None: the model's default, the bf16 speed mode).

    Examples::

        from ieee_amd import FeatureExtractor
        extractor = FeatureExtractor(model_name='ieee3modalPart', model_path='log/model.pth.tar-60')
        features = extractor([rgb_paths, ni_paths, ti_paths])       # (len(rgb_paths), 2304)
    """

    def __init__(self, model_name='ieee3modalPart', model_path='', image_size=(256, 128), pixel_mean=IMAGENET_MEAN,
                 pixel_std=IMAGENET_STD, pixel_norm=True, device='cuda', verbose=True, model=None, batch_size=64,
                 compute_dtype=None):
        global _said_unpretrained
        if int(batch_size) < 1:
            raise ValueError('batch_size must be at least 1, got {}'.format(batch_size))
        self.device = torch.device(device)
        if model is None:
            import os.path as osp
            from . import checkpoint
            from .models import build_model
            pretrained = checkpoint.find_resnet50_file() is not None
            if not pretrained and not _said_unpretrained:
                _said_unpretrained = True
                print('FeatureExtractor: {} is not on this machine: the backbones are built unpretrained'.format(
                    checkpoint.RESNET50_FILE))
            kwargs = {} if compute_dtype is None else {'compute_dtype': compute_dtype}
            model = build_model(model_name, num_classes=1, pretrained=pretrained,
                                use_gpu=self.device.type == 'cuda', **kwargs)
            if model_path and osp.isfile(model_path):
                checkpoint.load_pretrained_weights(model, model_path)
            model.to(self.device)
        else:
            model_name = type(model).__name__
        model.eval()
        if verbose:
            print('Model: {}'.format(model_name))
            print('- params: {:,}'.format(sum(p.numel() for p in model.parameters())))
        if not pixel_norm:
            pixel_mean, pixel_std = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
        self.model = model
        self.batch_size = int(batch_size)
        self.preprocess = DeviceTransform(image_size[0], image_size[1], [], norm_mean=pixel_mean, norm_std=pixel_std,
                                          train=False, device=None if self.device.index is None else self.device)

    @staticmethod
    def _member(member):
        """one modality's input -> a list of paths and uint8 HxWx3 arrays, or a float tensor [B, 3, H, W]"""
        if isinstance(member, (str, np.ndarray)):
            return [member]
        if isinstance(member, list):
            for element in member:
                if not isinstance(element, (str, np.ndarray)):
                    raise TypeError('Type of each element must belong to [str | numpy.ndarray]')
            return member
        if isinstance(member, torch.Tensor):
            return member.unsqueeze(0) if member.dim() == 3 else member
        raise TypeError('Type of each element must belong to [str | numpy.ndarray]')

    def _chunk(self, member, lo, hi):
        """rows lo .. hi of one modality, padded to batch_size rows with copies of row hi - 1, preprocessed, on the device
        (paths are decoded here, a chunk at a time)"""
        pad = self.batch_size - (hi - lo)
        if torch.is_tensor(member):
            x = member[lo:hi].to(self.device)
            return torch.cat([x, x[-1:].expand(pad, -1, -1, -1)]).contiguous() if pad else x.contiguous()
        from PIL import Image
        images = [np.asarray(Image.open(e).convert('RGB')) if isinstance(e, str) else e for e in member[lo:hi]]
        return self.preprocess.ragged(images + [images[-1]] * pad)

    def __call__(self, input):
        if not isinstance(input, (list, tuple)) or len(input) != 3:
            raise ValueError('expected the triple [RGB, NI, TI], got {}'.format(
                '{} members'.format(len(input)) if isinstance(input, (list, tuple)) else type(input)))
        members = [self._member(m) for m in input]
        counts = [len(m) for m in members]
        if counts[0] != counts[1] or counts[0] != counts[2]:
            raise ValueError('the three modalities must hold the same number of images, got {} RGB, {} NI, {} TI'.format(*counts))
        n = counts[0]
        features = []
        with torch.no_grad():
            for lo in range(0, n, self.batch_size):
                hi = min(lo + self.batch_size, n)
                f = self.model([self._chunk(m, lo, hi) for m in members])
                features.append(f[:hi - lo])
        if not features:
            return torch.empty((0, 2304), dtype=torch.float32, device=self.device)
        return features[0] if len(features) == 1 else torch.cat(features)
