"""The class behind the reference's looping-video / generative-frame-interpolation demo
(scripts/gradio/i2v_test_application.py): `Image2Video` with `get_image(..., image2=None)`. Everything said in i2v_test.py holds;
what differs is the c_concat latent - zeros except frame 0 = the image's latent and frame -1 = the second image's (or the first
again: a loop) - and that a loop drops its last decoded frame, which repeats the first. The reference loads the `_interp_v1`
checkpoints for this class; pass them as `ckpt_path=`.
"""
from . import i2v_test


class Image2Video(i2v_test.Image2Video):
    def _concat_cond(self, z, z2, frames):
        """i2v_test_application.py:80-89."""
        cc = z.new_zeros((z.shape[0], z.shape[1], frames) + tuple(z.shape[3:]))
        cc[:, :, :1] = z
        cc[:, :, -1:] = z if z2 is None else z2
        return cc

    def get_image(self, image, prompt, steps=50, cfg_scale=7.5, eta=1.0, fs=3, seed=123, image2=None, **sample_kwargs):
        """i2v_test_application.py:37-116. image, image2: uint8 [H, W, 3] ndarrays. Without `image2` the clip is a loop of
        temporal_length - 1 frames; with it, temporal_length frames from `image` to `image2`. Returns the path written."""
        return self._generate(image, prompt, steps, cfg_scale, eta, fs, seed, image2=image2, drop_last=image2 is None,
                              **sample_kwargs)
