"""cqs_amd — MI355X-native (gfx950) hot path of cqs: exact scan + top-k, embedding forward.

Product code lives here and in cqs_amd/csrc (HIP kernels + C ABI, include/cqs_hip.h).
It never imports anything from oracle/ (test infrastructure).
"""
from .index import (BackendContext, DiffEntry, DiffResult, DistanceMetric, DriftEntry, DriftResult, HipBackend, HipError,
                    HipIndex, IndexResult, MovedEntry, VectorIndex, merge_keys, prepare_index_data, tag_filter, unpack_keys)

__all__ = ["BackendContext", "DiffEntry", "DiffResult", "DistanceMetric", "DriftEntry", "DriftResult", "HipBackend", "HipError",
           "HipIndex", "IndexResult", "MovedEntry", "VectorIndex", "merge_keys", "prepare_index_data", "tag_filter", "unpack_keys"]
