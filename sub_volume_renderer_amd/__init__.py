"""MI355X-native sub-volume LMIP ray-march renderer.

Drop-in for the hot path of gyoge0/sub_volume_renderer: the same
``SubVolume`` / ``SubVolumeMaterial`` / ``WrappingBuffer`` surface
(reference ``src/sub_volume/__init__.py:9-21``) over a C ABI (``include/svr.h``)
implemented by hand-written HIP kernels for gfx950.  There is no CPU fallback:
device work raises if ``csrc/libsvr_hip.so`` has not been built.
"""

from ._geometry import Coordinate, Roi
from .compose import compose
from .outline import outline
from ._material import SubVolumeMaterial
from ._transfer import TransferFunction
from ._transform import AffineTransform, OrthographicCamera, PerspectiveCamera
from ._wobject import FrameRegion, HistogramResult, IsoResult, ObjectTable, RenderResult, SliceResult, SubVolume
from ._wrapping_buffer import WrappingBuffer, subtract_rois
from .mesh import SurfaceMesh
from .components import ComponentLabels
from .distance import DistanceField
from .nearest import NearestField
from .contacts import ContactTable
from .split import SplitLabels

__all__ = [
    "SubVolume",
    "SubVolumeMaterial",
    "TransferFunction",
    "WrappingBuffer",
    # replacements for what the reference imports from funlib.geometry / pygfx
    "Roi",
    "Coordinate",
    "PerspectiveCamera",
    "OrthographicCamera",
    "AffineTransform",
    "FrameRegion",
    "RenderResult",
    "SliceResult",
    "IsoResult",
    "HistogramResult",
    "ObjectTable",
    "SurfaceMesh",
    "ComponentLabels",
    "DistanceField",
    "NearestField",
    "ContactTable",
    "SplitLabels",
    "subtract_rois",
    # display-side output of a render (pygfx's job in the reference)
    "compose",
    "outline",
]
