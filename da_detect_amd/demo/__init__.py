"""The reference's demo/ by its names: `from da_detect_amd.demo.predictor import COCODemo`."""
