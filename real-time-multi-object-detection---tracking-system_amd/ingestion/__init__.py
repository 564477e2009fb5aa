from .reader import FrameReader, RTSPReader, RawVideoCapture, SyntheticCapture, register_backend  # noqa: F401
from .jpeg_decode import JpegDecodeError, JpegDecoder  # noqa: F401
from .mjpeg import MjpegCapture  # noqa: F401
from .lens import LensCorrector, fisheye_map, monotonic_r2  # noqa: F401
from .stabilizer import Stabilizer  # noqa: F401
from .health import CameraHealth  # noqa: F401
from .enhance import FrameEnhancer  # noqa: F401
from .denoise import FrameDenoiser  # noqa: F401

register_backend("mjpeg", MjpegCapture)          # FrameReader("x.avi", backend="mjpeg"): Motion-JPEG decoded on the GPU
