"""The slot-grouped text formats (``SPARSE_BINARY``, ``SPARSE``; ``pstext.hip``) under the
names their first callers used. The parser is ops/textparse.py ``parse_text_device``."""
from .textparse import parse_text_device as parse_ps_text_device  # noqa: F401
from .textparse import traits


def supported(fmt) -> bool:
    """Whether ``fmt`` (name or data.TEXT_FORMATS id) is parsed by the kernels of pstext.hip."""
    t = traits(fmt)
    return t is not None and t.family == "pstext"
