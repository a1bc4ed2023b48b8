from . import search  # noqa: F401  (registers the search kinds' parameter struct beside the others)
