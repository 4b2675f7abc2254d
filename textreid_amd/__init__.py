from .index import GalleryIndex  # noqa: F401
