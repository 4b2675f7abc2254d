from .index import GalleryIndex  # noqa: F401
from .index_shards import GalleryShards  # noqa: F401
