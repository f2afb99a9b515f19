"""Utilities on top of the likelihood path (the reference's pastml.utilities)."""
