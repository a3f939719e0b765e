"""torchreid-style model registry - mirror of modification_tracking/models/__init__.py:26-121.

The reference's registry maps ~55 names to torchreid constructors that are not vendored; its
own additions are 'vit' and 'swin_transformer' (:79-80).  This registry holds the backbones that exist as HIP
kernel sequences; every other name raises the same ``KeyError`` the reference raises for an unknown model.
"""
from .backbone import cares18_ibn, emares18_ibn, seres18_ibn, swin_t

__model_factory = {
    'seres18_ibn': seres18_ibn,
    'cares18_ibn': cares18_ibn,          # sibling backbones of reid/backbones (CARes18.py, EMA_Res18.py)
    'emares18_ibn': emares18_ibn,
    'swin_transformer': swin_t,          # the reference's own addition (models/__init__.py:80)
}
# build_model's own keywords -> the names that take them; every other name refuses a value other than None
__keyword_models = {
    'version': ('swin_transformer',),
    'hw_precision': ('seres18_ibn', 'cares18_ibn', 'emares18_ibn'),
    'hw_siblings': ('cares18_ibn',),
    'hw_ema': ('emares18_ibn',),
    'hw_f16': ('seres18_ibn',),
    'hw_sib_f16': ('cares18_ibn', 'emares18_ibn'),
}


def show_avai_models():
    print(list(__model_factory.keys()))


def build_model(name, num_classes, loss='softmax', pretrained=True, use_gpu=True, precision=None, version=None, hw_precision=None, hw_siblings=None, hw_ema=None, hw_f16=None, hw_sib_f16=None):
    """Same signature, same ``KeyError`` text as models/__init__.py:93-121; constructors are called with
    (num_classes, loss, pretrained, use_gpu).  ``precision`` (keyword, this engine's addition): the arithmetic the model runs
    in - None = $REID_PRECISION, else "f16x3", the mode bench.py reports (precision.py).  ``version`` (keyword): "v1" / "v2" of
    'swin_transformer', the reference's ``swin_t(..., version=)`` (image_reid_inference.py:202-208); other names take none.
    ``hw_precision`` (keyword): 'seres18_ibn' at inputs other than 256 x 128 - None = exact fp32 for such a call, "f16x3" = the fp32-class
    arithmetic (backbone.SERes18IBN); the Swin takes none.
    ``hw_siblings`` (keyword): True lets 'cares18_ibn' take inputs other than 256 x 128 too (backbone.CARes18IBN, Engine.set_hw_siblings);
    every other name takes none.  ``hw_ema`` (keyword): the same for 'emares18_ibn' (backbone.EMARes18IBN, Engine.set_hw_ema).
    ``hw_f16`` (keyword): True runs 'seres18_ibn' at inputs other than 256 x 128 in fp16 storage with fp32 accumulation (backbone.SERes18IBN,
    Engine.set_hw_f16); every other name takes none.  ``hw_sib_f16`` (keyword): True runs 'cares18_ibn' / 'emares18_ibn' at inputs other than
    256 x 128 in fp16 storage with fp32 accumulation (Engine.set_hw_sib_f16; the keyword alone is enough, and it goes without ``hw_precision``
    and ``hw_f16``); every other name takes none."""
    avai_models = list(__model_factory.keys())
    if name not in avai_models:
        raise KeyError('Unknown model: {}. Must be one of {}'.format(name, avai_models))
    extra = {}
    given = (('version', version), ('hw_precision', hw_precision), ('hw_siblings', hw_siblings), ('hw_ema', hw_ema), ('hw_f16', hw_f16),
             ('hw_sib_f16', hw_sib_f16))
    for keyword, value in given:
        if value is not None:
            if name not in __keyword_models[keyword]:
                raise ValueError("model '{}' has no {} argument".format(name, keyword))
            extra[keyword] = value
    return __model_factory[name](num_classes=num_classes, loss=loss, pretrained=pretrained, use_gpu=use_gpu, precision=precision, **extra)
