function setClipPlanes(r, planes)
% setClipPlanes  Cut-away views: clip planes for the renders of a VolumeRender object.
%
%   setClipPlanes(r, planes)   % planes: n x 4, rows [n0 n1 n2 offset], n <= 6
%   setClipPlanes(r, [])       % no planes: the whole volume again
%
% A plane keeps the half-space  n0*q0 + n1*q1 + n2*q2 + offset >= 0  of the normalized volume
% coordinate q: q(j) runs from 0 to 1 across dimension j of VolumeEmission.Data, the centre of voxel i
% (1-based) lying at (i - 0.5) / size(Data, j).  The kept region is the intersection of the planes and
% of the volume; six planes make a crop box.  Examples for a volume Data(d0, d1, d2):
%   setClipPlanes(r, [1 0 0 -0.5])                    % keep the upper half of dimension 1
%   setClipPlanes(r, [1 0 0 -0.25; -1 0 0 0.75])      % keep the slab 0.25 <= q0 <= 0.75
%
% No volume data changes and nothing is uploaded: a plane only shortens each ray, so a cut can move
% from frame to frame at the cost of the render alone.  The planes stay with the object's handle until
% the next setClipPlanes; they are honoured by r.render() (mono and stereo), renderProjection,
% renderIsosurface (a cut object shows a capped cut face) and renderTransfer.  renderChannels and
% handles that span several GPUs (VR_DEVICES) refuse to render while planes are set.  A clipped
% r.render() runs the general kernel instead of the staged march: several times the unclipped frame's
% time when little is cut away, less the more is (renderTransfer without lights and renderIsosurface
% stay fast).
% (volumeRender('set_clip', h, planes'), vr_set_clip in include/vrhip.h.)
if nargin < 2 || isempty(planes)
    volumeRender('set_clip', r.objectHandle, []);
    return;
end
if ~ismatrix(planes) || size(planes, 2) ~= 4
    error('planes must be an n x 4 matrix with rows [n0 n1 n2 offset].');
end
volumeRender('set_clip', r.objectHandle, single(planes'));
end
