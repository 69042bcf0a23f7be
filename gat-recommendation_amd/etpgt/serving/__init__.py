"""Serving on the HIP path: one request (``recommend``) or a batch of
them with the graphs built on the device (``recommend_batch``)."""

from etpgt.serving.recommender import Recommender, ValidatedRequest

__all__ = ["Recommender", "ValidatedRequest"]
