"""The anisotropic camera of the fx != fy tests.  Inputs only.

Every other case of the suite uses K_KITTI (fx == fy) or a uniform scaling of it, so a kernel
that read fx where it should read fy would pass them all.  K_ANISO has four distinct values, fy
about 0.91 fx, and a principal point inside both 1242x375 and 931x281 frames."""

K_ANISO = (721.5377, 655.25, 601.25, 183.5)
BF_ANISO = 352.0

# the dict form scene.SequenceRenderer(K=...) takes
K_ANISO_DICT = dict(fx=K_ANISO[0], fy=K_ANISO[1], cx=K_ANISO[2], cy=K_ANISO[3], bf=BF_ANISO)
# 3/4 resolution (931x281), as the small drives of the suite scale scene.KITTI03
K_ANISO_34_DICT = {k: v * 0.75 for k, v in K_ANISO_DICT.items()}
K_ANISO_34 = tuple(K_ANISO_34_DICT[k] for k in ("fx", "fy", "cx", "cy"))
BF_ANISO_34 = K_ANISO_34_DICT["bf"]


def swap_fxfy(K):
    """K with fx and fy exchanged: the camera a kernel with one fx/fy slip would effectively use.
    A case whose expected output does not change under this swap proves nothing."""
    return (K[1], K[0], K[2], K[3])
