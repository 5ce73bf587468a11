classdef RawVolume < Volume
% RawVolume  A Volume whose voxels stay in their native integer type until they are on the GPU.
%
%   v = RawVolume(h5read(file, dataset));          % uint8, uint16 or int16 data
%   v = RawVolume(data, true);                     % Unorm: uint8 -> [0, 1] (x / 255), uint16 (x / 65535)
%   render.VolumeEmission = v;                     % VolumeRender's setters take it: isa(v, 'Volume')
%
% Volume casts every dataset to single (Volume.m:78,89), so a volume crosses the host link at four
% bytes per voxel.  A RawVolume keeps the integer array in RawData; the volumeRender MEX reads
% RawData (and Unorm) when it is not empty, sends it in its own width, and widens it to single on
% the device during the upload.  The resident volume and every image are bit for bit those of
%   Volume(single(RawData))                        % Unorm = false
%   Volume(single(RawData) / single(255))          % Unorm = true, uint8 (65535 for uint16)
% Unorm is for uint8 and uint16 only (the MEX reports an error for int16).  The illumination LUT and
% the gradient volumes must stay single Volumes.
%
% Data (inherited) holds a 1x1 single placeholder and is not read while RawData is set; the
% Volume methods that work on Data (resize, normalize, grad, mip, ...) do not apply to RawData --
% use Volume(single(v.RawData)) for those.  Setting RawData stamps TimeLastUpdate, which is what
% the renderer's upload deduplication keys on.
%
% Not run here (written without a MATLAB installation); the MEX side of it is tested through the
% MEX stand-in (tests/test_mex_typed_volumes.py).

    properties
        % RawData: uint8, uint16 or int16 array (2-D or 3-D); empty: the object behaves as a Volume
        RawData = [];
        % Unorm: logical, true: voxel = single(RawData) / single(intmax(class(RawData)))
        Unorm = false;
    end

    methods
        function this = RawVolume(data, varargin)
            this = this@Volume(single(0));
            if nargin >= 2
                this.Unorm = varargin{1};
            end
            this.RawData = data;
        end

        function set.RawData(obj, data)
            if ~isempty(data) && ~(isa(data, 'uint8') || isa(data, 'uint16') || isa(data, 'int16'))
                error('RawVolume:type', 'RawData must be uint8, uint16 or int16');
            end
            if ndims(data) > 3
                error('RawVolume:dims', 'RawData must have at most 3 dimensions');
            end
            obj.RawData = data;
            obj.TimeLastUpdate = timestamp;
        end

        function set.Unorm(obj, value)
            obj.Unorm = logical(value);
            obj.TimeLastUpdate = timestamp;
        end

        function s = size(obj)
            if isempty(obj.RawData)
                s = size@Volume(obj);
            else
                s = size(obj.RawData);
            end
        end
    end
end
