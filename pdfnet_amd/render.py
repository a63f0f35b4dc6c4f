"""The two hand meshes in the image plane: the interface of the reference's `mano_two_hands_renderer` (lib/models/networks/mano_utils.py:105-191,
used by demo.py:84,283-291) over the HIP rasteriser of csrc/render.hip (`functional.render_hands`).  Perspective camera from a 3 x 3 intrinsic
matrix and per-vertex colours only: the reference's orthographic `scale` / `trans2d` camera and its UV textures are not built."""
import torch

from . import functional as F

LEFT_COLOUR, RIGHT_COLOUR = (92.0, 73.0, 179.0), (150.0, 161.0, 105.0)          # mano_utils.py:130-137, on the 0 .. 255 scale
LEFT_MASK, RIGHT_MASK = (0.0, 0.0, 255.0), (0.0, 255.0, 0.0)                    # render_mask: left hand blue, right hand green


class HandRenderer:
    def __init__(self, faces_pair, img_size):
        """faces_pair [2, Fc, 3] (left, right: the loss module's `faces_pair`) on the device that will render; img_size: a side or (H, W)."""
        self.faces = faces_pair.detach().long().contiguous()
        self.size = (int(img_size), int(img_size)) if isinstance(img_size, int) else tuple(int(s) for s in img_size)
        self._tables = {}

    def _table(self, n):
        if n not in self._tables:                                  # host-built, once per vertex count
            self._tables[n] = F.vertex_face_table(self.faces, n)
        return self._tables[n]

    def _colours(self, left, right, n, like):
        c = torch.tensor([left, right], dtype=torch.float32, device=like.device)                 # [2, 3]
        return c[:, None, :].expand(2, n, 3).contiguous()

    def _verts(self, v3d_left, v3d_right):
        return torch.stack((v3d_left, v3d_right), -3)              # [..., 2, n, 3]

    def render_rgb(self, cameras, v3d_left, v3d_right, v_color=None, amblights=False):
        """cameras [B, 3, 3], v3d_left / v3d_right [B, n, 3] camera-space metres, v_color [2n, 3] or [B, 2n, 3] on the 0 .. 255 scale (left hand's
        vertices first; default: the reference's two hand colours) -> (img [B, H, W, 3] = shaded colours / 255, alpha [B, H, W] = 1 where a
        hand covers the pixel)."""
        v = self._verts(v3d_left, v3d_right)
        n = v.shape[-2]
        if v_color is None:
            colour = self._colours(LEFT_COLOUR, RIGHT_COLOUR, n, v)
        else:
            colour = torch.as_tensor(v_color, dtype=torch.float32, device=v.device)
            colour = colour.reshape(colour.shape[:-2] + (2, n, 3))
        face, _, rgb = F.render_hands(v, self.faces, cameras, self.size, colour=colour, table=None if amblights else self._table(n),
                                      ambient_only=amblights)
        return rgb / 255, (face >= 0).float()

    def render_mask(self, cameras, v3d_left, v3d_right):
        """-> img [B, H, W, 3]: the left hand's pixels (0, 0, 1), the right hand's (0, 1, 0), ambient light only."""
        v = self._verts(v3d_left, v3d_right)
        colour = self._colours(LEFT_MASK, RIGHT_MASK, v.shape[-2], v)
        return F.render_hands(v, self.faces, cameras, self.size, colour=colour, ambient_only=True)[2] / 255

    def render_depth(self, cameras, v3d_left, v3d_right):
        """-> depth [B, H, W]: Z of the visible surface in metres, 0 where there is none."""
        return F.render_hands(self._verts(v3d_left, v3d_right), self.faces, cameras, self.size)[1]

    @staticmethod
    def overlay(img_out, alpha, image):
        """img_out, image [..., H, W, 3] on one scale, alpha [..., H, W] -> img_out * alpha + image * (1 - alpha) (demo.py:289)."""
        mask = alpha[..., None]
        return img_out * mask + image * (1 - mask)
