"""evals/models/maskcut_processor.py of the reference, on the HIP path: the class lives in mvp/maskcut.py."""
from mvp.maskcut import MaskCutProcessor

__all__ = ["MaskCutProcessor"]
