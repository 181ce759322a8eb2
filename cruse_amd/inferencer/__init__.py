from .base_inferencer import Inferencer  # noqa: F401
from .streaming import StreamingInferencer  # noqa: F401
