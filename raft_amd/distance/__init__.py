from .pairwise import pairwise_distance, pack_bits, DistanceType

__all__ = ["pairwise_distance", "pack_bits", "DistanceType"]
