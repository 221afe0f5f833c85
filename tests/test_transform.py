"""Hand-derived known answers for the camera conventions both the product and the oracle consume
(``_transform.py``; in the reference these matrices come from pygfx / pylinalg, absent here).  The parity
tests feed the SAME matrices to both sides, so a wrong convention would be invisible to them: these pins
are what stands in for that."""
import numpy as np

import pytest

from sub_volume_renderer_amd._transform import AffineTransform, OrthographicCamera, PerspectiveCamera


def test_projection_matrix_fov_applies_to_the_mean_extent_and_depth_maps_to_0_1():
    # pygfx PerspectiveCamera: the field of view spans the MEAN of the view's width and height.
    # fov 90 deg, aspect 2, near 1, far 3:  mean extent at the near plane = 2 * near * tan(45 deg) = 2
    #   height = 2 * 2 / (1 + aspect) = 4/3,  width = aspect * height = 8/3  (mean = 2)
    #   right = 4/3, top = 2/3
    cam = PerspectiveCamera(90.0, 2.0, depth_range=(1.0, 3.0))
    want = np.array([[1.0 / (4.0 / 3.0), 0, 0, 0],
                     [0, 1.0 / (2.0 / 3.0), 0, 0],
                     [0, 0, 3.0 / (1.0 - 3.0), 1.0 * 3.0 / (1.0 - 3.0)],
                     [0, 0, -1.0, 0]])
    np.testing.assert_allclose(cam.projection_matrix, want, rtol=0, atol=1e-12)
    P = cam.projection_matrix
    # the near plane's top-right corner -> NDC (1, 1, 0); a far-plane point on the axis -> z = 1 (wgpu depth [0, 1])
    c = P @ np.array([4.0 / 3.0, 2.0 / 3.0, -1.0, 1.0])
    np.testing.assert_allclose(c[:3] / c[3], [1.0, 1.0, 0.0], atol=1e-12)
    c = P @ np.array([0.0, 0.0, -3.0, 1.0])
    np.testing.assert_allclose(c[2] / c[3], 1.0, atol=1e-12)
    np.testing.assert_allclose(cam.projection_matrix_inverse @ P, np.eye(4), atol=1e-12)


def test_projection_matrix_square_view_is_the_textbook_frustum():
    cam = PerspectiveCamera(60.0, 1.0, depth_range=(0.5, 100.0))
    f = 1.0 / np.tan(np.radians(30.0))
    P = cam.projection_matrix
    np.testing.assert_allclose([P[0, 0], P[1, 1]], [f, f], rtol=1e-12)
    np.testing.assert_allclose(P[2, 2], 100.0 / (0.5 - 100.0))
    np.testing.assert_allclose(P[2, 3], 0.5 * 100.0 / (0.5 - 100.0))
    cam.zoom = 2.0                                        # zoom narrows the extent
    np.testing.assert_allclose(cam.projection_matrix[0, 0], 2 * f, rtol=1e-12)


def test_look_at_points_local_minus_z_at_the_target_with_y_up():
    cam = PerspectiveCamera(45.0, 1.0)
    cam.world.position = (1.0, 2.0, 3.0)
    cam.look_at((1.0, 2.0, -5.0))                         # straight down -z: no rotation at all
    np.testing.assert_allclose(cam.world.rotation_matrix, np.eye(3), atol=1e-12)
    cam.look_at((11.0, 2.0, 3.0))                         # down +x: local -z = +x, local y stays +y, local x = +z... right-handed
    R = cam.world.rotation_matrix
    np.testing.assert_allclose(R @ np.array([0, 0, -1.0]), [1, 0, 0], atol=1e-12)
    np.testing.assert_allclose(R @ np.array([0, 1.0, 0]), [0, 1, 0], atol=1e-12)
    np.testing.assert_allclose(np.linalg.det(R), 1.0, atol=1e-12)
    # view matrix = inverse of the camera's world matrix: the eye maps to the origin, the target onto -z
    V = cam.view_matrix
    np.testing.assert_allclose(V @ np.array([1.0, 2.0, 3.0, 1.0]), [0, 0, 0, 1], atol=1e-12)
    np.testing.assert_allclose(V @ np.array([11.0, 2.0, 3.0, 1.0]), [0, 0, -10, 1], atol=1e-12)


def test_affine_transform_composes_translate_rotate_scale():
    t = AffineTransform()
    t.position = (1.0, 2.0, 3.0)
    t.scale = (1.0, 1.0, 6.0)                             # scripts/mouse.py:90-91 (world.scale_z = 6)
    np.testing.assert_allclose(t.matrix @ np.array([1.0, 1.0, 1.0, 1.0]), [2, 3, 9, 1])
    np.testing.assert_allclose(t.inverse_matrix @ t.matrix, np.eye(4), atol=1e-12)
    assert t.scale_z == 6.0


# ---- orthographic camera (pygfx OrthographicCamera conventions) ---------------------------------------------------
def _ortho_want(w, h, near, far):
    """x, y: [-w/2, w/2] x [-h/2, h/2] -> [-1, 1]^2;  view z = -near -> 0, view z = -far -> 1;  w = 1."""
    return np.array([[2.0 / w, 0, 0, 0],
                     [0, 2.0 / h, 0, 0],
                     [0, 0, -1.0 / (far - near), -near / (far - near)],
                     [0, 0, 0, 1.0]])


@pytest.mark.parametrize("w,h,aspect,maintain,zoom,want_wh", [
    (16.0, 16.0, 1.0, True, 1.0, (16.0, 16.0)),          # square extent, square frame
    (16.0, 16.0, 1.0, False, 1.0, (16.0, 16.0)),
    (20.0, 10.0, 2.0, True, 1.0, (20.0, 10.0)),          # non-square extent that already has the frame's ratio
    (20.0, 10.0, 1.0, True, 1.0, (20.0, 20.0)),          # frame squarer than the extent: the height grows
    (20.0, 10.0, 4.0, True, 1.0, (40.0, 10.0)),          # frame wider than the extent: the width grows
    (20.0, 10.0, 1.0, False, 1.0, (20.0, 10.0)),         # maintain_aspect off: stretched, nothing grows
    (20.0, 10.0, 4.0, False, 1.0, (20.0, 10.0)),
    (16.0, 8.0, 2.0, True, 2.0, (8.0, 4.0)),             # zoom 2 halves the extent
    (16.0, 8.0, 1.0, True, 0.5, (32.0, 32.0)),           # zoom 1/2 doubles it, then the height grows to the ratio
])
def test_orthographic_projection_known_answers(w, h, aspect, maintain, zoom, want_wh):
    cam = OrthographicCamera(w, h, aspect, zoom=zoom, maintain_aspect=maintain, depth_range=(2.0, 10.0))
    assert cam.extent == want_wh
    P = cam.projection_matrix
    np.testing.assert_array_equal(P, _ortho_want(*want_wh, 2.0, 10.0))      # every entry exact (powers of two etc.)
    np.testing.assert_allclose(cam.projection_matrix_inverse @ P, np.eye(4), atol=1e-12)
    # the corners of the visible extent at the near plane -> NDC (+-1, +-1, 0); on the far plane z = 1
    hw, hh = want_wh[0] / 2.0, want_wh[1] / 2.0
    for sx in (-1.0, 1.0):
        for sy in (-1.0, 1.0):
            np.testing.assert_allclose(P @ np.array([sx * hw, sy * hh, -2.0, 1.0]), [sx, sy, 0.0, 1.0], atol=1e-12)
            np.testing.assert_allclose(P @ np.array([sx * hw, sy * hh, -10.0, 1.0]), [sx, sy, 1.0, 1.0], atol=1e-12)


def test_orthographic_depth_is_linear_and_w_is_one_everywhere():
    cam = OrthographicCamera(12.0, 6.0, 2.0, depth_range=(-4.0, 12.0))     # near plane 4 units BEHIND the camera
    P = cam.projection_matrix
    rng = np.random.default_rng(0)
    pts = np.concatenate([rng.uniform(-50, 50, (200, 3)), np.ones((200, 1))], axis=1)
    c = pts @ P.T
    np.testing.assert_array_equal(c[:, 3], 1.0)                             # no perspective divide at all
    np.testing.assert_allclose(c[:, 2], (-pts[:, 2] + 4.0) / 16.0, rtol=0, atol=1e-12)     # linear in distance
    assert (P @ np.array([0, 0, 4.0, 1]))[2] == 0.0                          # near plane (behind the camera)
    assert (P @ np.array([0, 0, -12.0, 1]))[2] == 1.0                        # far plane
    # x / y do not depend on depth: parallel rays
    a, b = P @ np.array([1.5, -2.0, -1.0, 1.0]), P @ np.array([1.5, -2.0, -11.0, 1.0])
    assert a[0] == b[0] == 0.25 and a[1] == b[1] == -2.0 / 3.0


def test_orthographic_camera_pose_conventions_match_the_perspective_camera():
    o, p = OrthographicCamera(8.0, 8.0, 1.0, depth_range=(1.0, 9.0)), PerspectiveCamera(45.0, 1.0, depth_range=(1.0, 9.0))
    for cam in (o, p):
        cam.world.position = (3.0, 4.0, 20.0)
        cam.look_at((3.0, 4.0, 0.0))
    np.testing.assert_array_equal(o.view_matrix, p.view_matrix)
    np.testing.assert_array_equal(o.camera_matrix, p.camera_matrix)
    # a point 5 units in front of the camera, 1 unit to its right and 2 up: NDC x = 1 / 4, y = 2 / 4, depth (5-1)/8
    c = o.projection_matrix @ o.view_matrix @ np.array([4.0, 6.0, 15.0, 1.0])
    np.testing.assert_allclose(c, [0.25, 0.5, 0.5, 1.0], atol=1e-12)


def test_orthographic_default_depth_range():
    """The default near / far (no depth_range) is restated and parity unpinned; this only pins what it is here."""
    cam = OrthographicCamera(10.0, 30.0)
    assert cam.near_far == (-20000.0, 20000.0)
    cam.depth = 2.0
    assert cam.near_far == (-2000.0, 2000.0)
