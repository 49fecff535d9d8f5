"""rustyhgi_amd -- MI355X-native (gfx950) HGI encode/decode core behind the surface of pl0q1n/RustyHGI.

Crate-root re-exports as in the reference's src/lib.rs:16-23:
    rustyhgi_amd.{Archive, Metadata, Decoder, Encoder}, rustyhgi_amd.interpolator, rustyhgi_amd.quantizator
plus rustyhgi_amd.entropy (device-side byte histogram of the grid) and rustyhgi_amd.Planes (device
buffers placed for MI355X's HBM regions, include/hgi.h hgi_planes_alloc) and rustyhgi_amd.mapping (the 256-entry tables of
Decoder.decode_mapped, include/hgi_map.h, and the constants of Encoder.encode_typed, include/hgi_typed.h).
Encoder.requantize re-codes stored grids with another table in one launch (libhgi_requant.so, include/hgi_requant.h).
rustyhgi_amd.views (ViewPlan, aligned_arena) plans view lists -- frames with a pitch of their own each -- for Encoder.encode_views /
Decoder.decode_views: one launch per list (libhgi_views.so, include/hgi_views.h).
rustyhgi_amd.mviews (MappedViewPlan, padded_batch) plans mapped view lists -- mixed-size grids decoded straight into float16 /
bfloat16 / float32 frames with a pitch of their own each -- for Decoder.decode_mapped_views: one launch per list
(libhgi_mviews.so, include/hgi_mviews.h).
rustyhgi_amd.tviews (TypedViewPlan) plans typed view lists -- mixed-size float16 / bfloat16 / float32 frames with a pitch of
their own each, encoded straight into grids -- for Encoder.encode_typed_views: one launch per list (libhgi_tviews.so,
include/hgi_tviews.h).
Encoder.requantize_views re-codes a view list of stored grids -- a ViewPlan of (source grid, destination grid) pairs, the plan
of the view lists unchanged -- with another table: one launch per list (libhgi_qviews.so, include/hgi_qviews.h).
rustyhgi_amd.sviews (ScaledViewPlan, scaled_shape) plans scaled view lists -- mixed-size stored grids decoded at 1 / 2**shift
resolution, each through pitches of its own -- for Decoder.decode_scaled_views: one launch per list (libhgi_sviews.so,
include/hgi_sviews.h).
rustyhgi_amd.rviews (ReconViewPlan) plans recon view lists -- mixed-size frames encoded into grids and into the images the
decoder will make of them, each through three pitches of its own -- for Encoder.encode_views_with_reconstruction: one launch
per list (libhgi_rviews.so, include/hgi_rviews.h).
All computation happens in libhgi_hip.so (hand-written HIP kernels); see include/hgi.h.
"""
from . import entropy, interpolator, mapping, mviews, quantizator, rviews, sviews, tviews, views
from ._ffi import Context, HgiError, default_context
from .archive import Archive, Metadata
from .codec import Decoder, Encoder
from .grid import Grid
from .mapping import affine_inverse, affine_table
from .mviews import MappedViewPlan, padded_batch
from .planes import Planes
from .rviews import ReconViewPlan
from .sviews import ScaledViewPlan, scaled_shape
from .tviews import TypedViewPlan
from .views import ViewPlan, aligned_arena

__all__ = ["Encoder", "Decoder", "Grid", "Archive", "Metadata", "Context", "HgiError", "default_context", "interpolator",
           "quantizator", "entropy", "Planes", "mapping", "affine_table", "affine_inverse", "views", "ViewPlan",
           "aligned_arena", "mviews", "MappedViewPlan", "padded_batch", "tviews", "TypedViewPlan", "sviews",
           "ScaledViewPlan", "scaled_shape", "rviews", "ReconViewPlan"]
