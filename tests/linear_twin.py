"""The linear sample (include/svr.h, "interpolation") under its name, and the four twins with it.  The definition is
the ``linear`` branch of ``twin_common.sample``; every twin takes ``linear=True`` and nothing else in its definition
changes, so the functions here only pass that argument."""
import functools

import composite_twin
import iso_twin
import slab_twin
import slice_twin
from twin_common import sample

linear_sample = functools.partial(sample, linear=True)          # (rings, dd, allowed=None) -> value, label, lod
slice_linear = functools.partial(slice_twin.slice_twin, linear=True)
slab_linear = functools.partial(slab_twin.slab_twin, linear=True)
composite_linear = functools.partial(composite_twin.composite_twin, linear=True)
iso_linear = functools.partial(iso_twin.iso_twin, linear=True)
slice_of_spec = functools.partial(slice_twin.twin_of_spec, linear=True)
slab_of_spec = functools.partial(slab_twin.twin_of_spec, linear=True)
