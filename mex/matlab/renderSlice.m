function [image, aux, labels] = renderSlice(r, varargin)
% renderSlice  A section through the resident volume: an axis-aligned or oblique slice, or a thick slab.
%
%   image = renderSlice(r, 'Axis', 3, 'Index', 40)                 % the voxel plane Data(:, :, 40)
%   image = renderSlice(r, 'Axis', 2, 'Index', 17, 'Thickness', 9, 'Mode', 'mean')
%   image = renderSlice(r, 'Point', [0.5 0.5 0.5], 'Normal', [1 1 0.5], 'Up', [0 0 1], ...
%                       'PixelSizeUm', 0.5, 'Resolution', [512 512])
%   [image, aux, labels] = renderSlice(r, ...)
%
% What the renderer samples -- a RawVolume widened to single, label gains applied -- evaluated with the
% renders' own trilinear sampler on a plane (volumeRender('render_slice', ...), vr_render_slice in
% include/vrhip.h).  No camera is involved, and clip planes are ignored: the slice is itself the cut.
%   'Axis', 'Index'   the voxel plane Index (1-based, fractions allowed) along dimension Axis (1-based) of
%                     Data: one pixel per voxel, the lower-numbered remaining dimension along the rows.
%   'Point', 'Normal', 'Up', 'PixelSizeUm', 'Resolution'
%                     the [H W] plane through Point (normalized volume coordinate q of the image centre,
%                     q(j) from 0 to 1 across dimension j of Data), orthonormal in physical space
%                     (ElementSizeUm): Normal and Up are physical directions, component j along dimension
%                     j; rows run along Up projected into the plane; pixels PixelSizeUm apart (default:
%                     the smallest element size); Resolution defaults to flip(ImageResolution).
%   'Thickness'       slab samples (default 1), one voxel resp. PixelSizeUm apart, centred.
%   'Mode'            'max' (default) | 'min' | 'mean' | 'sum' over the slab's samples inside the volume.
%   'Source'          'emission' (default) | 'absorption' | 'reflection'.
% image is single [H W], NaN where no sample lies inside the volume; aux is the index of the extremum
% (0-based) resp. the number of inside samples; labels is the label at the slab's centre sample (NaN
% outside, or without labels).
p = inputParser;
addParameter(p, 'Axis', []);
addParameter(p, 'Index', []);
addParameter(p, 'Point', []);
addParameter(p, 'Normal', []);
addParameter(p, 'Up', []);
addParameter(p, 'PixelSizeUm', []);
addParameter(p, 'Resolution', []);
addParameter(p, 'Thickness', 1);
addParameter(p, 'Mode', 'max');
addParameter(p, 'Source', 'emission');
parse(p, varargin{:});
o = p.Results;
if all([islogical(r.VolumeReflection), islogical(r.VolumeAbsorption), islogical(r.VolumeEmission)])
    error('Not all volumes are properly set!');
end
switch lower(o.Source)
    case 'emission',   vol = r.VolumeEmission;
    case 'absorption', vol = r.VolumeAbsorption;
    case 'reflection', vol = r.VolumeReflection;
    otherwise, error('Source must be ''emission'', ''absorption'' or ''reflection''.');
end
d = [size(vol.Data, 1), size(vol.Data, 2), size(vol.Data, 3)];
t = double(o.Thickness);
if ~isempty(o.Axis)
    ax = o.Axis;
    rest = setdiff(1:3, ax);             % rows along rest(1), columns along rest(2)
    first = (double(o.Index) - 1) - (t - 1) / 2;
    origin = zeros(3, 1); du = zeros(3, 1); dv = zeros(3, 1); dw = zeros(3, 1);
    origin(ax) = (first + 0.5) / d(ax);   dw(ax) = 1 / d(ax);
    origin(rest(1)) = 0.5 / d(rest(1));   dv(rest(1)) = 1 / d(rest(1));
    origin(rest(2)) = 0.5 / d(rest(2));   du(rest(2)) = 1 / d(rest(2));
    res = [d(rest(1)), d(rest(2))];
else
    if isempty(o.Point) || isempty(o.Normal)
        error('Give ''Axis'' and ''Index'', or ''Point'' and ''Normal''.');
    end
    es = double(r.ElementSizeUm);
    ext = d(:) .* [es(3); es(2); es(1)];   % ElementSizeUm(4 - j) belongs to dimension j
    w = double(o.Normal(:)); w = w / norm(w);
    if isempty(o.Up)
        up = zeros(3, 1); [~, k] = min(abs(w)); up(k) = 1;
    else
        up = double(o.Up(:));
    end
    v = up - (up' * w) * w;
    if norm(v) < 1e-9 * norm(up) || norm(up) == 0
        error('Up is parallel to the normal.');
    end
    v = v / norm(v);
    u = cross(v, w);
    px = o.PixelSizeUm; if isempty(px), px = min(es); end
    res = o.Resolution; if isempty(res), res = flip(r.ImageResolution); end
    du = u * px ./ ext; dv = v * px ./ ext; dw = w * px ./ ext;
    origin = double(o.Point(:)) - (res(2) - 1) / 2 * du - (res(1) - 1) / 2 * dv - (t - 1) / 2 * dw;
end
mode = lower(o.Mode);
isMean = strcmp(mode, 'mean');
if isMean, mode = 'sum'; end
r.syncVolumes();
[image, aux, labels] = volumeRender('render_slice', r.objectHandle, single([origin, du, dv, dw]), ...
    uint64(res), t, mode, lower(o.Source));
if isMean
    image = image ./ aux;
end
end
