from .views import complex_view, fix_dim, window_view  # noqa: F401
