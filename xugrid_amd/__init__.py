"""
xugrid_amd -- MI355X-native engine for xugrid's regridding hot path (weight construction and the
sparse weight x data apply), behind the reference's own Regridder API.  See DESIGN.md.

The compute path is hand-written HIP for gfx950 in ``xugrid_amd/csrc`` exposed through the C ABI
of ``include/xugrid_amd.h``; this package is the thin Python host side.  There is no CPU
fallback: without ``libxugrid_amd.so`` and a HIP device every compute call raises.
"""
from . import engine, meshgen  # noqa: F401
from ._lib import XugridAmdError  # noqa: F401
from .burn import burn_vector_geometry, locate_polygon  # noqa: F401
from .celltree import CellTree2d  # noqa: F401
from .fill import laplace_interpolate  # noqa: F401
from .geometry import unique_xy  # noqa: F401
from . import connectivity  # noqa: F401
from .graph import binary_dilation, binary_erosion, connected_components, reverse_cuthill_mckee  # noqa: F401
from .partition import label_partitions, labels_to_indices, merge_partitions, partition_by_label  # noqa: F401
from .polygonize import polygonize  # noqa: F401
from .regrid import (  # noqa: F401
    BarycentricInterpolator,
    CentroidLocatorRegridder,
    LayeredGrid,
    LayeredOverlapRegridder,
    LayeredRelativeOverlapRegridder,
    NetworkGridder,
    OverlapRegridder,
    Raster,
    RelativeOverlapRegridder,
    overlap_1d_nd,
)
from .snap import snap_nodes, snap_to_nodes  # noqa: F401
from .snapgrid import create_snap_to_grid_dataframe, snap_to_grid  # noqa: F401
from .sparse import MatrixCOO, MatrixCSR  # noqa: F401
from .topology import DeviceTopology  # noqa: F401
from .ugrid1d import Ugrid1d  # noqa: F401
from .ugrid2d import Ugrid2d  # noqa: F401

__version__ = "0.1.0"
