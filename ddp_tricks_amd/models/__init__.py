from .convnext import convnext_tiny  # noqa: F401
from .mnasnet import mnasnet1_0  # noqa: F401
from .mobilenet import mobilenet_v1  # noqa: F401
from .resnet import (  # noqa: F401
    resnet18, resnet34, resnet50, resnext50_32x4d, resnext101_32x8d,
    se_resnet50, se_resnext50_32x4d,
)
from .toy_net import Toy_Net  # noqa: F401
from .vgg import vgg16_bn  # noqa: F401
from .vit import vit_small, vit_tiny  # noqa: F401

_REGISTRY = {
    "toy_net": Toy_Net,
    "resnet18": resnet18,
    "resnet34": resnet34,
    "resnet50": resnet50,
    "resnext50_32x4d": resnext50_32x4d,
    "resnext101_32x8d": resnext101_32x8d,
    "se_resnet50": se_resnet50,
    "se_resnext50_32x4d": se_resnext50_32x4d,
    "vgg16": vgg16_bn,
    "mobilenet_v1": mobilenet_v1,
    "mnasnet1_0": mnasnet1_0,
    "convnext_tiny": convnext_tiny,
    "vit_tiny": vit_tiny,
    "vit_small": vit_small,
}


def build_model(name: str, **kwargs):
    try:
        return _REGISTRY[name](**kwargs)
    except KeyError:
        raise ValueError(f"unknown model {name!r}; available: {sorted(_REGISTRY)}")


def model_accepts(name: str, kwarg: str) -> bool:
    """Whether the registered constructor takes ``kwarg`` by name."""
    import inspect
    try:
        ctor = _REGISTRY[name]
    except KeyError:
        raise ValueError(f"unknown model {name!r}; available: {sorted(_REGISTRY)}")
    params = inspect.signature(ctor).parameters
    return kwarg in params or any(
        p.kind is inspect.Parameter.VAR_KEYWORD for p in params.values())


def register_model(name: str, ctor) -> None:
    _REGISTRY[name] = ctor
