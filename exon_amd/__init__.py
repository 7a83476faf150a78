"""exon_amd -- MI355X-native scan -> filter -> aggregate path for Exon-style genomic Arrow data.

The product is the HIP library `exon_amd/lib/libexon_hip.so` behind the C ABI of `include/exon_hip.h`;
this package is the thin host side used by tests, the CLI and bench.py.  Importing the operators
fails loudly when the library is missing -- there is no CPU fallback.
"""
from ._lib import ExonHipError, LIB_PATH, build, load  # noqa: F401
from .engine import (Context, DeviceBuffer, Plan, RegionSetPlan, RegionBasesPlan, WindowBasesPlan, RegionDepthPlan, Scan, Stream, VCFParser, FASTQParser, FASTAParser, BAMParser, BCFParser, SAMParser, GFFParser, BEDParser, bgzf_scan, index_query, minmax_decode, parse_region,  # noqa: F401
                     read_stats_layout, region_bases_decode, region_bases_layout, region_set_decode, region_set_layout, regroup_files_by_size, seq_stats_layout, cigar_blocks_host)  # noqa: F401
from ._lib import REGION_BASES_LDS_MAX, REGION_SET_LDS_MAX, WINDOW_BASES_LDS_MAX, REGION_DEPTH_LDS_MAX, REGION_DEPTH_REDUCE_TILE, REGION_DEPTH_MAX_BINS, COVER_ALIGNED, COVER_ALIGNED_DEL  # noqa: F401

__all__ = ["Context", "DeviceBuffer", "Plan", "Scan", "Stream", "ExonHipError", "parse_region", "index_query",
           "regroup_files_by_size", "minmax_decode", "read_stats_layout", "seq_stats_layout", "RegionSetPlan", "region_set_layout", "region_set_decode", "REGION_SET_LDS_MAX", "RegionBasesPlan", "region_bases_layout", "region_bases_decode", "REGION_BASES_LDS_MAX", "WindowBasesPlan", "WINDOW_BASES_LDS_MAX", "RegionDepthPlan", "REGION_DEPTH_LDS_MAX", "REGION_DEPTH_REDUCE_TILE", "REGION_DEPTH_MAX_BINS", "cigar_blocks_host", "COVER_ALIGNED", "COVER_ALIGNED_DEL", "build", "load", "LIB_PATH"]
