"""`COCODemo`: one image in, the image with its detections drawn out — by the names of the reference's demo/predictor.py, so
the loop of its demo/draw_detection.py runs with nothing changed but the import.

What is kept by name: the constructor's arguments, `build_transform`, `compute_prediction`, `select_top_predictions`,
`compute_colors_for_labels`, `overlay_boxes`, `overlay_class_names`, `run_on_opencv_image`, `CATEGORIES`.  What differs:
  * no cv2 and no torchvision: the image is resized, reordered and normalised by this package's device input pipeline
    (data/device_prep.py, the arithmetic of Pillow's bilinear resize), and drawn by engine/overlay.py — on the device
    (csrc/overlay.hip) when the model lives there;
  * text is drawn with this project's 6 x 11 glyph cells on a plate in the box colour, as "{name} {score:.2f}", not with
    cv2's Hershey strokes in a fixed colour;
  * boxes are painted by ascending score, the most confident one on top (the reference paints it first);
  * mask heat maps, mask contours and keypoints are not on this path: asking for them raises NotImplementedError;
  * `CATEGORIES` is the COCO name list in COCO's own order (the reference's copy carries the Cityscapes names in places
    2 .. 8); pass `categories=` for any other label set, e.g. ("__background__",) + data.cityscapes.CATEGORIES.
`run_on_image` is the RGB form of `run_on_opencv_image`; the methods named after the reference take BGR arrays, as cv2 would
have delivered them, unless called with rgb=True."""
import numpy as np
import torch

from ..data.device_prep import DeviceBatchPreparer
from ..engine import overlay
from ..modeling.detector import build_detection_model
from ..utils.checkpoint import DetectronCheckpointer


class COCODemo(object):
    CATEGORIES = [
        "__background", "person", "bicycle", "car", "motorcycle", "airplane", "bus", "train", "truck", "boat",
        "traffic light", "fire hydrant", "stop sign", "parking meter", "bench", "bird", "cat", "dog", "horse", "sheep",
        "cow", "elephant", "bear", "zebra", "giraffe", "backpack", "umbrella", "handbag", "tie", "suitcase", "frisbee",
        "skis", "snowboard", "sports ball", "kite", "baseball bat", "baseball glove", "skateboard", "surfboard",
        "tennis racket", "bottle", "wine glass", "cup", "fork", "knife", "spoon", "bowl", "banana", "apple", "sandwich",
        "orange", "broccoli", "carrot", "hot dog", "pizza", "donut", "cake", "chair", "couch", "potted plant", "bed",
        "dining table", "toilet", "tv", "laptop", "mouse", "remote", "keyboard", "cell phone", "microwave", "oven",
        "toaster", "sink", "refrigerator", "book", "clock", "vase", "scissors", "teddy bear", "hair drier", "toothbrush",
    ]

    def __init__(self, cfg, confidence_threshold=0.7, min_image_size=224, categories=None, show_mask_heatmaps=False,
                 masks_per_dim=2):
        if show_mask_heatmaps:
            raise NotImplementedError("mask heat maps: the mask head is not on this path")
        if cfg.MODEL.MASK_ON or cfg.MODEL.KEYPOINT_ON:
            raise NotImplementedError("MODEL.MASK_ON / MODEL.KEYPOINT_ON: only the box head is on this path")
        self.cfg = cfg.clone()
        self.model = build_detection_model(cfg)
        self.model.eval()
        self.device = torch.device(cfg.MODEL.DEVICE)
        self.model.to(self.device)
        self.min_image_size = min_image_size
        DetectronCheckpointer(cfg, self.model, save_dir=cfg.MODEL.OUTPUT_DIR).load(cfg.MODEL.WEIGHT)  # (this tree keeps it there)
        self.transforms = self.build_transform()
        self.cpu_device = torch.device("cpu")
        self.confidence_threshold = confidence_threshold
        self.show_mask_heatmaps = show_mask_heatmaps
        self.masks_per_dim = masks_per_dim
        if categories is not None:
            self.CATEGORIES = list(categories)

    # ------------------------------------------------------------------------------------------------------ the input
    def build_transform(self):
        """predictor.py:143-171 — shorter side to `min_image_size` (torchvision's Resize with one integer), TO_BGR255,
        normalise — as a callable over uint8 [H, W, 3] RGB device pixels -> ImageList padded to SIZE_DIVISIBILITY"""
        preparer = DeviceBatchPreparer(self.cfg, is_train=False)
        size = int(self.min_image_size)

        def transform(pixels_u8):
            h, w = int(pixels_u8.shape[0]), int(pixels_u8.shape[1])
            if w <= h:
                out = (h if w == size else int(size * h / w), size)
            else:
                out = (size, w if h == size else int(size * w / h))
            images, _ = preparer([pixels_u8], None, decisions=[(out, False)])
            return images

        return transform

    def _upload(self, image, rgb):
        image = np.asarray(image)
        assert image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3, "uint8 [H, W, 3] image expected"
        if not rgb:
            image = image[:, :, ::-1]
        return torch.from_numpy(np.ascontiguousarray(image)).to(self.device)

    def compute_prediction(self, original_image, rgb=False):
        """image (uint8 [H, W, 3] array; BGR unless rgb=True) -> BoxList on the CPU, resized to the image's own size"""
        pixels = original_image if isinstance(original_image, torch.Tensor) else self._upload(original_image, rgb)
        with torch.no_grad():
            predictions = self.model(self.transforms(pixels))
        prediction = predictions[0].to(self.cpu_device)
        height, width = int(pixels.shape[0]), int(pixels.shape[1])
        return prediction.resize((width, height))

    # ---------------------------------------------------------------------------------------------------- the drawing
    def select_top_predictions(self, predictions):
        return overlay.select_top_predictions(predictions, self.confidence_threshold)

    def compute_colors_for_labels(self, labels):
        return overlay.compute_colors_for_labels(labels)

    def draw_list(self, predictions):
        return overlay.build_draw_list(predictions, self.CATEGORIES)

    def _render(self, image, records, rgb):
        image = np.asarray(image)
        if not rgb:
            image = image[:, :, ::-1]
        if self.device.type == "cuda":
            pixels = torch.from_numpy(np.ascontiguousarray(image)).to(self.device)
            out = overlay.render_device([pixels], [records])[0].cpu().numpy()
        else:
            out = overlay.render_host(image, records)
        return out if rgb else np.ascontiguousarray(out[:, :, ::-1])

    def overlay_boxes(self, image, predictions, rgb=False):
        """predictor.py:264-285: the boxes of `predictions` on a copy of `image`"""
        return self._render(image, overlay.boxes_only(self.draw_list(predictions)), rgb)

    def overlay_class_names(self, image, predictions, rgb=False):
        """predictor.py:358-383: the labels of `predictions` on a copy of `image`"""
        return self._render(image, overlay.labels_only(self.draw_list(predictions)), rgb)

    def run_on_opencv_image(self, image):
        """BGR array, as cv2 would have delivered it -> BGR array with the detections above the threshold drawn"""
        return np.ascontiguousarray(self.run_on_image(np.asarray(image)[:, :, ::-1])[:, :, ::-1])

    def run_on_image(self, image_rgb):
        """RGB array -> RGB array with the detections above the threshold drawn.  The pixels are uploaded once: the
        detector's input is prepared from them and the overlay drawn onto a copy of them."""
        pixels = self._upload(image_rgb, rgb=True)
        records = self.draw_list(self.select_top_predictions(self.compute_prediction(pixels)))
        if self.device.type != "cuda":
            return overlay.render_host(np.asarray(image_rgb), records)
        return overlay.render_device([pixels.clone()], [records])[0].cpu().numpy()
