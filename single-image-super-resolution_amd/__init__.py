"""MI355X-native (gfx950) SRGAN training hot path with the module interface of
keyber/Single-Image-Super-Resolution.  See DESIGN.md / INTEGRATION.md at the repository root.

The package directory name contains hyphens, so import it with
``importlib.import_module("single-image-super-resolution_amd")`` (or put ``dropin/`` on
``sys.path`` to get ``model_generator`` / ``model_discriminator`` / ``model_content_extractor`` under the
reference's own module names; ``install()`` additionally patches ``utils.lr_from_hr``).
"""
from . import _lib  # noqa: F401

_FILTERS = ('gaussian_taps', 'gaussian_blur', 'usm_sharpen', 'USMSharp')      # filters.py
_RESIZE = ('resize', 'resize_taps', 'expected_resize_modes')                   # resize.py
_ARTIFACT = ('artifact_map', 'artifact_loss')                                  # losses.py
_PERCEP = ('gram_matrix', 'perceptual_loss', 'PerceptualLoss')                 # losses.py
_CONTEXTUAL = ('contextual_loss', 'contextual_similarity', 'ContextualLoss')     # losses.py
_NIQE = ('niqe', 'niqe_features', 'NiqeModel')                                 # metrics.py


def __getattr__(name):
    """the public names of ``filters`` and ``resize``, the artifact-aware, perceptual and contextual losses of ``losses`` and the no-reference score
    of ``metrics`` under the package's own name, resolved on first use (importing the package stays light)"""
    if name in _FILTERS:
        import importlib
        return getattr(importlib.import_module('.filters', __name__), name)
    if name in _ARTIFACT or name in _PERCEP or name in _CONTEXTUAL:
        import importlib
        return getattr(importlib.import_module('.losses', __name__), name)
    if name in _NIQE:
        import importlib
        return getattr(importlib.import_module('.metrics', __name__), name)
    if name in _RESIZE:                         # ``resize`` itself is the (callable) module: that is what the name is bound to from then on
        import importlib
        mod = importlib.import_module('.resize', __name__)
        return mod if name == 'resize' else getattr(mod, name)
    raise AttributeError('module %r has no attribute %r' % (__name__, name))


def install(fused_adam=False, fused_losses=False, degradation=None):
    """Register this package's model modules under the reference's top-level module names, so the
    reference's ``train.py`` / ``config.py`` import them unchanged, and point ``utils.lr_from_hr`` -- the one hot
    function of the reference's ``utils`` module (utils.py:22-31; called at train.py:46,96, config.py:272) -- at the
    HIP kernel.  The reference's own ``utils`` module is NOT shadowed: its plotting / checkpoint helpers
    (``save_and_show``, ``save_curr_vis``, ``SamplerRange`` ... train.py:15,36, config.py:250) stay the reference's;
    only when no ``utils`` module is importable at all (this repository's own tests) is the package's ``utils``
    registered under that name.  ``fused_adam=True`` also points ``torch.optim.Adam`` (what config.py:293-294
    instantiates) at the fused multi-tensor Adam of ``optim.py``; ``fused_losses=True`` points ``torch.nn.BCELoss`` (what
    config.py:107 instantiates) at the fused ``losses.BCELoss``; ``degradation=`` a ``degrade.Degrader`` makes the patched
    ``utils.lr_from_hr`` that object's method -- a blur kernel and a noise level drawn per sample and per call
    -- instead of the bicubic kernel (``Degrader(jpeg=(qlo, qhi))`` appends the JPEG round trip of ``jpeg.py``, DESIGN.md section 20;
    a ``degrade.HighOrderDegrader`` is taken the same way: Real-ESRGAN's second-order model);
    the default None leaves the bicubic path as it is."""
    import importlib
    import sys
    if fused_adam:
        import torch
        torch.optim.Adam = importlib.import_module('.optim', __name__).Adam
    if fused_losses:
        import torch
        torch.nn.BCELoss = importlib.import_module('.losses', __name__).BCELoss
    for name in ('model_generator', 'model_generator_progressive', 'model_discriminator', 'model_content_extractor'):
        sys.modules[name] = importlib.import_module('.' + name, __name__)
    ours = importlib.import_module('.utils', __name__)
    try:
        ref_utils = importlib.import_module('utils')          # the reference's utils.py, when it is on the path
    except ImportError:
        sys.modules['utils'] = ref_utils = ours
    if ref_utils is not ours:
        ref_utils.lr_from_hr = ours.lr_from_hr
        ref_utils._subsampling_interpolation = ours._subsampling_interpolation
    if degradation is not None:
        ref_utils.lr_from_hr = degradation.lr_from_hr
