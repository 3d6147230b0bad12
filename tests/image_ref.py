"""NumPy restatement of the two conversions the camera-image calls do on the device (csrc/k_image.hip, the uint8 form of
k_conv3x3_first): OpenCV's 8-bit colour-to-gray and the float input of the NetVLAD network.

gray: cv2.cvtColor(image, COLOR_RGB2GRAY / COLOR_BGR2GRAY) on CV_8U [upstream OpenCV; not in the reference tree, restated
from memory: DESIGN.md section 3] is (R kr + G kg + B kb + (1 << (shift - 1))) >> shift in int32, with
  rule 0, OpenCV 3.x: 4899, 9617, 1868, shift 14      rule 1, OpenCV 4.x: 9798, 19235, 3735, shift 15
netvlad_input: the reference feeds its uint8 rgb8 image to a float32 placeholder (data_handler.py:60-61, 149-154): the
values 0 .. 255 unscaled, channels in R, G, B order."""
import numpy as np

RGB8, BGR8, MONO8 = 0, 1, 2
RULES = {0: (4899, 9617, 1868, 14), 1: (9798, 19235, 3735, 15)}     # (kr, kg, kb, shift)


def gray(img, format, rule=0):
    """img: uint8 [..., 3] (rgb8 / bgr8) or [...] (mono8) -> uint8 [...]."""
    img = np.asarray(img, np.uint8)
    if format == MONO8:
        return img.copy()
    kr, kg, kb, shift = RULES[rule]
    c = img.astype(np.int32)
    r, b = (c[..., 0], c[..., 2]) if format == RGB8 else (c[..., 2], c[..., 0])
    return ((r * np.int32(kr) + c[..., 1] * np.int32(kg) + b * np.int32(kb) + np.int32(1 << (shift - 1))) >> shift).astype(np.uint8)


def netvlad_input(img, format):
    """uint8 [h, w, 3] (rgb8 / bgr8) or [h, w] (mono8) -> float32 [h, w, 3], R, G, B."""
    img = np.asarray(img, np.uint8)
    if format == MONO8:
        return np.repeat(img[..., None], 3, axis=-1).astype(np.float32)
    return np.ascontiguousarray(img[..., ::-1] if format == BGR8 else img).astype(np.float32)
