# Same file name as the reference experiment config (README.md:58-64); inherits the path keys.
_base_ = ["../base.py"]
out_path = "out/plangen/h_text_ump+oimsam"
use_special_tokens = True              # h_text_ump+oimsam.py:11: the six layout tags are single tokens, as the checkpoint was trained
